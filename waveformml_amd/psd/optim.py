"""``FlatSGD``: torch.optim.SGD whose update of ONE flat fp32 GPU parameter is a single HIP launch
(include/wfsparse.h, wfs_sgd_step).  Drop-in for the optimizer the reference's configs name
(``"optimizer_class": "optim.SGD"``, config/examples/GEP.json:51-69; built at src/engineering/LitPSD.py:60-76):
same constructor, same ``state_dict`` layout (``momentum_buffer``), same arithmetic; anything it does not cover
(several tensors, CPU tensors, ``maximize``, closures) falls back to torch's own step.

``FlatAdam`` / ``FlatAdamW``: the same for torch.optim.Adam / AdamW (wfs_adam_step), state ``step`` / ``exp_avg`` /
``exp_avg_sq`` / ``max_exp_avg_sq`` as torch keeps it, ``step`` on the parameter's device.

The learning rate (Adam: every hyperparameter) lives in device memory, so a scheduler can change
``param_groups[i]["lr"]`` between replays of a captured HIP graph: call ``sync_hyperparameters()``
(psd/graph.GraphedTrainStep does) and the next replay uses it.  Flat optimizers always step inside the graph
(psd/graph.steps_in_graph).
"""
import torch

from .. import _lib


class FlatSGD(torch.optim.SGD):
    flat_device_step = True

    def _fast_groups(self):
        for g in self.param_groups:
            ps = g["params"]
            if (len(ps) != 1 or not ps[0].is_cuda or ps[0].dtype != torch.float32 or not ps[0].is_contiguous()
                    or g.get("maximize", False) or g.get("differentiable", False)):
                return False
        return True

    def sync_hyperparameters(self):
        """Copy each group's current ``lr`` to its device scalar if it changed (one tiny fill, only then)."""
        for g in self.param_groups:
            dev = g["params"][0].device
            if g.get("_lr_dev") is None or g["_lr_dev"].device != dev:
                g["_lr_dev"] = torch.empty((1,), dtype=torch.float32, device=dev)
                g["_lr_host"] = None
            if g["_lr_host"] != float(g["lr"]):
                g["_lr_dev"].fill_(float(g["lr"]))
                g["_lr_host"] = float(g["lr"])

    def state_dict(self):
        sd = super().state_dict()
        for g in sd["param_groups"]:
            g.pop("_lr_dev", None)
            g.pop("_lr_host", None)
        sd["state"] = {k: {n: v for n, v in st.items() if n != "_fresh"} for k, st in sd["state"].items()}
        return sd

    def mark_fresh(self):
        """The momentum buffers exist (a captured graph holds their addresses) but carry no history: the next EAGER
        step treats them as torch treats a missing buffer (buf = g, no dampening).  Only matters with dampening != 0 --
        with dampening 0 a zeroed buffer gives the same first step."""
        for g in self.param_groups:
            if g["dampening"] != 0 and g["momentum"] != 0:
                for p in g["params"]:
                    if "momentum_buffer" in self.state.get(p, {}):
                        self.state[p]["_fresh"] = True

    def has_fresh(self):
        return any(st.get("_fresh", False) for st in self.state.values())

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None or not self._fast_groups():
            return super().step(closure)
        lib = _lib.load()
        self.sync_hyperparameters()
        for g in self.param_groups:
            p = g["params"][0]
            if p.grad is None:
                continue
            grad = p.grad
            if grad.is_sparse or grad.dtype != torch.float32 or not grad.is_contiguous():
                return super().step(closure)
            state = self.state[p]
            buf, first = state.get("momentum_buffer"), False
            if g["momentum"] != 0 and buf is None:
                buf = state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                first = True
            if state.pop("_fresh", False) and not torch.cuda.is_current_stream_capturing():
                first = True
            _lib.check(lib.wfs_sgd_step(_lib.ptr(p), _lib.ptr(grad), _lib.ptr(buf) if g["momentum"] != 0 else None,
                                        p.numel(), _lib.ptr(g["_lr_dev"]), float(g["momentum"]), float(g["dampening"]),
                                        float(g["weight_decay"]), 1 if g["nesterov"] else 0, 1 if first else 0,
                                        _lib.stream_ptr()))
        return None


_ADAM_COEF_FLOATS = 16          # include/wfsparse.h WFS_ADAM_COEF_FLOATS


class _FlatAdamStep(object):
    """The HIP step of FlatAdam / FlatAdamW.  Per group, a device block of five doubles (lr, beta1, beta2, eps,
    weight_decay) and the kernel's coefficient workspace live on the optimizer, not in the groups: ``state_dict()`` is
    torch's, and a ``load_state_dict()`` keeps the addresses a captured graph holds."""
    flat_device_step = True

    def _fast_groups(self):
        for g in self.param_groups:
            ps = g["params"]
            if (len(ps) != 1 or not ps[0].is_cuda or ps[0].dtype != torch.float32 or not ps[0].is_contiguous()
                    or torch.is_tensor(g["lr"]) or g.get("differentiable", False)):
                return False
        return True

    @staticmethod
    def _hyper(g):
        beta1, beta2 = g["betas"]
        return (float(g["lr"]), float(beta1), float(beta2), float(g["eps"]), float(g["weight_decay"]))

    def sync_hyperparameters(self):
        """Write each group's changed hyperparameters to its device block (one tiny fill per changed value, only then).
        A value changed while the stream is capturing raises: a fill captured into the graph would write the capture-time
        value back at every replay."""
        dev_blocks = self.__dict__.setdefault("_flat_dev", {})
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        for i, g in enumerate(self.param_groups):
            dev = g["params"][0].device
            blk = dev_blocks.get(i)
            if blk is None or blk[0].device != dev:
                if capturing:
                    raise RuntimeError("FlatAdam: the first step runs outside a graph capture (it allocates the "
                                       "hyperparameter block)")
                blk = dev_blocks[i] = [torch.empty((5,), dtype=torch.float64, device=dev),
                                       torch.zeros((_ADAM_COEF_FLOATS,), dtype=torch.float32, device=dev), [None] * 5]
            hyper, _, host = blk
            for k, v in enumerate(self._hyper(g)):
                if host[k] != v:
                    if capturing:
                        raise RuntimeError("FlatAdam: a hyperparameter changed during a graph capture; call "
                                           "sync_hyperparameters() before capturing and before every replay")
                    hyper[k:k + 1].fill_(v)
                    host[k] = v
        return dev_blocks

    def load_state_dict(self, state_dict):
        """torch's load, then ``step`` goes to the parameter's device (torch keeps a non-capturable Adam's on the CPU)."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state.get(p)
                if st and torch.is_tensor(st.get("step")) and st["step"].device != p.device:
                    st["step"] = st["step"].to(device=p.device, dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None or not self._fast_groups():
            return super().step(closure)
        work = [g for g in self.param_groups if g["params"][0].grad is not None]
        for g in work:
            grad = g["params"][0].grad
            if grad.is_sparse or grad.dtype != torch.float32 or not grad.is_contiguous():
                return super().step(closure)
        capturing = torch.cuda.is_current_stream_capturing()
        lib = _lib.load()
        dev_blocks = self.sync_hyperparameters()
        for i, g in enumerate(self.param_groups):
            p = g["params"][0]
            if p.grad is None:
                continue
            st = self.state[p]
            names = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if g["amsgrad"] else [])
            if "step" not in st or any(k not in st for k in names) or st["step"].device != p.device:
                if capturing:
                    raise RuntimeError("FlatAdam: the optimizer state is created outside a graph capture (run one "
                                       "step, or load a state, before capturing)")
                if "step" not in st:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["step"] = st["step"].to(device=p.device, dtype=torch.float32)
                for k in names:
                    if k not in st:
                        st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
            hyper, coef, _ = dev_blocks[i]
            _lib.check(lib.wfs_adam_step(_lib.ptr(p), _lib.ptr(p.grad), _lib.ptr(st["exp_avg"]),
                                         _lib.ptr(st["exp_avg_sq"]), _lib.ptr(st.get("max_exp_avg_sq")) if g["amsgrad"]
                                         else None, p.numel(), _lib.ptr(hyper), _lib.ptr(st["step"]), _lib.ptr(coef),
                                         1 if g["amsgrad"] else 0, 1 if g["maximize"] else 0,
                                         1 if g.get("decoupled_weight_decay", False) else 0, _lib.stream_ptr()))
        return None


class FlatAdam(_FlatAdamStep, torch.optim.Adam):
    """torch.optim.Adam (same constructor and state); the update of one flat fp32 GPU tensor is wfs_adam_step."""


class FlatAdamW(_FlatAdamStep, torch.optim.AdamW):
    """torch.optim.AdamW (same constructor and state); the update of one flat fp32 GPU tensor is wfs_adam_step."""
