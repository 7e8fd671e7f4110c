"""Inference-only loops of the PSD path.

``test_loop``        what ``pytorch_lightning.Trainer.test(runner, datamodule)`` does for the reference's Evaluate.py
                     (Evaluate.py:69-84): eval mode, no gradients, ``LitPSD.test_step`` per batch (which zeroes feature
                     column ``occlude_index`` when it is set, src/engineering/LitPSD.py:130-151), event-weighted means.
``segment_test_loop`` the same for the per-segment regression modules (psd/litz.LitZ, LitEZ): ``test_step`` per batch,
                     row-weighted mean losses, the batch's dense maps handed to a psd/segment_evaluator evaluator.  Also
                     the loop of LitSegClassifier (PIDEvaluator) and of LitWaveform (TensorEvaluator).
``occlusion_sweep``  the reference's occlusion study (scripts/RunOcclusionStudy.py) runs Evaluate.py once per feature
                     index, i.e. re-reads the data and rebuilds every rulebook for each index although the geometry of a
                     batch never changes.  Here ONE batch already in HBM is run through the net for a list of indices
                     with its rulebooks built once (spconv.ops.reuse_rulebooks); only the feature column differs.
"""
import torch

from ..spconv import ops
from .data import to_device
from .eval_common import FIXED_ONE

_HEAD = 4       # class_metrics.HEAD's rows counted, rows correct, loss rows, loss sum


def _score(module, logits, labels):
    """test_loss / test_acc of reference LitPSD.test_step (:136-141) from the logits."""
    loss = module.criterion.forward(logits, labels)
    pred = torch.argmax(module.softmax(logits), dim=1)
    return loss.detach().float(), (pred == labels).float().mean()          # device scalars: no host sync per batch


def _tables_score(module, metrics):
    """Whether ``metrics``' tables give test_loss / test_acc as ``_score`` does: the criterion is an unweighted,
    mean-reduced ``CrossEntropyLoss`` without label smoothing whose ``ignore_index`` is the tables'."""
    c = module.criterion
    return (metrics is not None and type(c) is torch.nn.CrossEntropyLoss and c.weight is None and c.reduction == "mean"
            and getattr(c, "label_smoothing", 0.0) == 0.0 and c.ignore_index == metrics.ignore_index)


def _reduce_tables(*owners):
    """One SUM all-reduce per persistent accumulator of every evaluator / metrics object that is not None."""
    import torch.distributed as dist
    for owner in owners:
        if owner is not None:
            for t in owner.state_tensors():              # integer tables (and fp64 pulse sums): sums over batches
                dist.all_reduce(t, op=dist.ReduceOp.SUM)


@torch.no_grad()
def test_loop(module, loader, device, feature_dtype=None, capture=False, evaluator=None, metrics=None):
    """``capture=True``: the forward runs as replays of one captured HIP graph (psd/graph.GraphedEvalStep); a batch that
    does not fit the captured capacities takes the ordinary ``test_step``.
    ``evaluator``: a psd/evaluator.PSDEvaluator; every batch is handed to its ``add`` with the logits and their argmax, as
    the reference's ``test_step`` does (src/engineering/LitPSD.py:142-150) -- on the stream the forward ran on, without a
    read-back -- and the returned dict gains ``"evaluation": evaluator.results()``.
    ``metrics``: a psd/class_metrics.ClassificationMetrics (``module.metrics``); every batch's logits and labels go to its
    ``add`` -- one launch on the forward's stream -- and the returned dict gains ``"metrics": metrics.results()``.  In
    the captured branch, under a plain mean-reduced ``CrossEntropyLoss`` (``_tables_score``), ``_score``'s chain of small
    launches is not run behind a replay: the tables are exact integers, so the replayed batches' sum of cross-entropy
    terms and count of correct rows are what the tables' head holds at the end less what it held at the start (and less
    what the batches that took the ordinary ``test_step`` added).  The sum stands for ``sum(loss_b * b)``, which it
    equals as long as no label is the criterion's ``ignore_index`` (LitPSD has one label per event)."""
    module.to(device)
    module.eval()
    tot, acc, n = 0.0, 0.0, 0          # tot / acc become device scalars: one read-back at the end of the loop
    step = None
    from_tables = capture and _tables_score(module, metrics)
    head0, n_tab = (metrics.tables[:_HEAD].clone(), 0) if from_tables else (None, 0)
    try:
        for i, batch in enumerate(loader):
            batch = to_device(batch, device, feature_dtype)
            b = int(batch[1].shape[0])
            if capture:
                if step is None:
                    from .graph import GraphedEvalStep
                    step = GraphedEvalStep(module, batch)
                if step.fits(batch):
                    logits = step(batch, module.occlude_index)
                    if metrics is not None:
                        metrics.add(logits, batch[1])
                    if from_tables:
                        n_tab += b
                    else:
                        loss, a = _score(module, logits, batch[1])
                        tot, acc, n = tot + loss * b, acc + a * b, n + b
                    if evaluator is not None:
                        # the static buffers hold the batch as the net saw it (occluded column included)
                        evaluator.add(([step.coords, step.feats, step.n_valid], step.labels), logits,
                                      torch.argmax(logits, dim=1))
                    continue
            res = module.test_step(batch, i)
            if evaluator is not None:
                logits = module.last_test_logits
                evaluator.add(batch, logits, torch.argmax(logits, dim=1))
            if metrics is not None:
                before = metrics.tables[:_HEAD].clone() if from_tables else None
                metrics.add(module.last_test_logits, batch[1], n_valid=module._unpack(batch)[2])
                if from_tables:
                    head0 += metrics.tables[:_HEAD] - before      # this batch is scored by test_step's own result
            tot = tot + res["test_loss"].detach().float() * b
            acc = acc + res["test_acc"].detach().float() * b
            n += b
        if step is not None:
            step.check()
    finally:
        if step is not None:
            step.close()
    if from_tables:
        head = (metrics.tables[:_HEAD] - head0).double()          # this rank's replayed batches, before any reduction
        tot = tot + head[3] / FIXED_ONE                           # class_metrics.HEAD: n, correct, loss rows, loss sum
        acc, n = acc + head[1], n + n_tab
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        # every rank ran its own share of the items (data.rank_sampler): event-weighted sums over all ranks
        sums = torch.stack([torch.as_tensor(tot, dtype=torch.float64, device=device).reshape(()),
                            torch.as_tensor(acc, dtype=torch.float64, device=device).reshape(()),
                            torch.tensor(float(n), dtype=torch.float64, device=device)])
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
        tot, acc, n = float(sums[0]), float(sums[1]), int(sums[2])
        _reduce_tables(evaluator, metrics)
    out = {"test_loss": float(tot) / max(n, 1), "test_acc": float(acc) / max(n, 1), "events": n}
    if evaluator is not None:
        out["evaluation"] = evaluator.results()
    if metrics is not None:
        out["metrics"] = metrics.results()
    return out


@torch.no_grad()
def segment_test_loop(module, loader, device, feature_dtype=None, evaluator=None, metrics=None):
    """``test_step`` of a LitZ / LitEZ per batch in eval mode; every ``test_*`` entry it returns comes back as its mean
    over batches weighted by the batch's rows (the segment losses are per-row means, src/engineering/LitBase.py:171).
    ``evaluator``: a psd/segment_evaluator ZEvaluator / EZEvaluator; every batch's (predictions, dense targets,
    coordinates, features) go to its ``add`` as in the reference's ``test_step`` (LitZ.py:134-141, LitEZ.py:86-89) -- on the
    stream the forward ran on, without a read-back -- and the returned dict gains ``"evaluation": evaluator.results()``.
    The loop only needs ``module.last_test_outputs`` to hold ``evaluator.add``'s arguments, so it serves
    psd/litseg.LitSegClassifier (PIDEvaluator) and psd/litwaveform.LitWaveform (psd/tensor_evaluator.TensorEvaluator:
    ``(c, f, target, per-row loss)``) as it stands.
    ``metrics``: a psd/class_metrics.ClassificationMetrics (``module.metrics`` of a LitSegClassifier); every batch's
    ``module.last_test_logits`` and labels go to its ``add`` with ``module.last_test_loss_mask`` (the single-ended rows
    under ``SELoss``) -- one launch on the forward's stream -- and the returned dict gains ``"metrics": metrics.results()``."""
    module.to(device)
    module.eval()
    sums, n = {}, 0
    for i, batch in enumerate(loader):
        batch = to_device(batch, device, feature_dtype)
        rows = int(batch[0][0].shape[0])
        res = module.test_step(batch, i)
        if evaluator is not None:
            evaluator.add(*module.last_test_outputs)
        if metrics is not None:
            metrics.add(module.last_test_logits, batch[1], n_valid=module._unpack(batch)[2],
                        loss_mask=getattr(module, "last_test_loss_mask", None))
        for k, v in res.items():
            sums[k] = sums.get(k, 0.0) + v.detach().double() * rows       # device scalars: one read-back at the end
        n += rows
    keys = sorted(sums)
    import torch.distributed as dist
    if keys and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        packed = torch.stack([sums[k].reshape(()) for k in keys] + [torch.tensor(float(n), dtype=torch.float64, device=device)])
        dist.all_reduce(packed, op=dist.ReduceOp.SUM)
        sums, n = {k: packed[j] for j, k in enumerate(keys)}, int(packed[-1])
        _reduce_tables(evaluator, metrics)
    out = {k: float(sums[k]) / max(n, 1) for k in keys}
    out["rows"] = n
    if evaluator is not None:
        out["evaluation"] = evaluator.results()
    if metrics is not None:
        out["metrics"] = metrics.results()
    return out


@torch.no_grad()
def occlusion_sweep(module, batch, occlude_indices, capture=False):
    """{index: {"test_loss", "test_acc"}} for one device-resident batch ``([coords, feats], labels)``.
    ``None`` in ``occlude_indices`` is the unoccluded pass.  Index 0 is passed through as it is: the reference's
    ``if self.occlude_index:`` treats it as "no occlusion" (LitPSD.py:134), and so does the mirror.
    ``capture=True``: one captured graph builds the batch's rulebooks and runs the first pass, a second, forward-only
    graph is replayed for every further index (psd/graph.GraphedEvalStep(sweep=True))."""
    (coords, feats), labels = batch
    module.eval()
    out = {}
    if capture and len(occlude_indices) > 0:
        from .graph import GraphedEvalStep
        step = GraphedEvalStep(module, batch, sweep=True)
        try:
            scores = []
            for n, idx in enumerate(occlude_indices):
                logits = step(batch, idx) if n == 0 else step.rerun(idx)
                scores.append(torch.stack(_score(module, logits, labels)))
            host = torch.stack(scores).cpu()              # one read-back for the whole sweep
            for idx, row in zip(occlude_indices, host):
                out[idx] = {"test_loss": float(row[0]), "test_acc": float(row[1])}
            step.check()
        finally:
            step.close()
        return out
    saved = module.occlude_index
    try:
        with ops.reuse_rulebooks():
            for idx in occlude_indices:
                module.occlude_index = idx
                res = module.test_step(([coords, feats.clone()], labels), 0)      # test_step zeroes the column in place
                out[idx] = {"test_loss": float(res["test_loss"]), "test_acc": float(res["test_acc"])}
    finally:
        module.occlude_index = saved
    return out
