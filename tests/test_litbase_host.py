"""psd/litbase.LitBase under the six Lightning-module mirrors (LitPSD, LitSegClassifier, LitSegQuantifier, LitZ, LitEZ,
LitWaveform), on the CPU: one definition of the shared methods, the module layout checkpoints were saved with
(tests/golden/lit_module_layout.json, written before the base existed), the keyword arguments each class hands its
evaluator, the optimizer each class configures, and the named refusal of a padded batch on LitZ."""
import json
import os

import pytest
import torch

import lit_layout_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "lit_module_layout.json")) as _f:
    GOLD = json.load(_f)
SIX = ["LitPSD", "LitSegClassifier", "LitSegQuantifier", "LitZ", "LitEZ", "LitWaveform"]
SHARED = ["log", "log_dict", "forward", "configure_optimizers"]
# the one expected difference from the recorded layout: LitSegQuantifier is no longer a LitPSD and so has lost the
# parameter-free LogSoftmax child it never used
LOST_CHILDREN = {"LitSegQuantifier": ["softmax"]}
_MODULES = {}


def _module(name):
    if name not in _MODULES:
        _MODULES[name] = lc.build(name)
    return _MODULES[name]


def test_one_definition():
    from waveformml_amd.psd.litbase import LitBase
    from waveformml_amd.psd.litz import LitSegmentBase
    classes = [lc.lit_class(name) for name in SIX]
    assert all(issubclass(cls, LitBase) for cls in classes + [LitSegmentBase])
    assert all(name in vars(LitBase) for name in SHARED)
    for cls in classes:
        for base in cls.__mro__[:cls.__mro__.index(LitBase)]:
            assert not set(SHARED) & set(vars(base)), (base, sorted(set(SHARED) & set(vars(base))))


@pytest.mark.parametrize("part", ["state_dict", "children", "buffers"])
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_layout_is_the_recorded_one(name, part):
    want = GOLD[name][part]
    if part == "children":
        lost = LOST_CHILDREN.get(name, [])
        assert all(c in want for c in lost)
        want = [c for c in want if c not in lost]
    assert lc.layout(_module(name))[part] == want
    assert set(GOLD) == set(lc.CASES)


def test_layout_record_covers_the_mask_and_the_order():
    """The record itself: ``model`` first, ``criterion`` second everywhere, and the per-segment cases carry SE_mask."""
    for name, rec in GOLD.items():
        assert rec["children"][:2] == ["model", "criterion"], name
    for name in ("LitSegClassifier", "LitSegQuantifier", "LitZ"):
        assert GOLD[name]["buffers"][0] == "SE_mask" and GOLD[name]["state_dict"][0] == ["SE_mask", [1, 1, 14, 11], "torch.float32"]


class Recorder:
    made = []

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs
        Recorder.made.append(self)


EVALUATORS = [("pid_evaluator", "PIDEvaluator"), ("quantifier_evaluator", "SegEvaluator"), ("segment_evaluator", "ZEvaluator"),
              ("segment_evaluator", "EZEvaluator"), ("real_z_evaluator", "ZEvaluatorRealWFNorm"),
              ("tensor_evaluator", "TensorEvaluator"), ("evaluator", "PSDEvaluator"), ("phys_evaluator", "PhysEvaluator")]


@pytest.fixture
def recorded(monkeypatch):
    """Every evaluator class replaced, at its source module, by one recorder class per name."""
    import importlib
    classes = {}
    for module, cls in EVALUATORS:
        classes[cls] = type(cls, (Recorder,), {})
        monkeypatch.setattr(importlib.import_module("waveformml_amd.psd." + module), cls, classes[cls])
    Recorder.made = []
    return classes


def _evaluator_of(name, classes, want_class, **sections):
    """Build case ``name`` with the given config sections merged in, read ``evaluator`` twice."""
    def edit(cfg):
        for section, values in sections.items():
            cfg.setdefault(section, {}).update(values)
    Recorder.made = []
    m = lc.build(name, edit)
    ev = m.evaluator
    assert type(ev) is classes[want_class] and m.evaluator is ev and Recorder.made == [ev]     # built once, then cached
    return m, ev


CPU = torch.device("cpu")
FIELDS = {"test_dataset_params": {"label_name": "phys", "additional_fields": ["PID"]}}


def test_segment_classifier_evaluator_keywords(recorded):
    # additional_field_names from the dataset, evaluation_config over it, then excludes -> dead_pmts
    _, ev = _evaluator_of("LitSegClassifier", recorded, "PIDEvaluator", dataset_config=FIELDS,
                          evaluation_config={"additional_field_names": ["x"], "excludes": [3, 5], "n_bins": 7})
    assert ev.args == (CPU,) and ev.kwargs == {"additional_field_names": ["x"], "n_bins": 7, "dead_pmts": [3, 5]}
    _, ev = _evaluator_of("LitSegClassifier", recorded, "PIDEvaluator", dataset_config=FIELDS)
    assert ev.kwargs == {"additional_field_names": ["PID"]}
    _, ev = _evaluator_of("LitSegClassifier", recorded, "PIDEvaluator")
    assert ev.kwargs == {}


def test_segment_quantifier_evaluator_keywords(recorded):
    # the same, then target_index (dataset_params.label_index = 4), whatever evaluation_config says
    _, ev = _evaluator_of("LitSegQuantifier", recorded, "SegEvaluator",
                          evaluation_config={"additional_field_names": ["x"], "excludes": [3, 5], "target_index": 9})
    assert ev.args == (CPU,)
    assert ev.kwargs == {"additional_field_names": ["x"], "dead_pmts": [3, 5], "target_index": 4}
    _, ev = _evaluator_of("LitSegQuantifier", recorded, "SegEvaluator")
    assert ev.kwargs == {"additional_field_names": ["PID"], "target_index": 4}        # the shipped config's fields


def test_litz_evaluator_keywords(recorded, monkeypatch):
    from waveformml_amd.psd import litz
    # phys targets: evaluation_config first, the dataset's fields written over it, excludes left alone
    m, ev = _evaluator_of("LitZ", recorded, "ZEvaluatorRealWFNorm", dataset_config=FIELDS,
                          evaluation_config={"additional_field_names": ["x"], "excludes": [1], "wf_analysis": True})
    assert m.test_has_phys and ev.args == (CPU,)
    assert ev.kwargs == {"additional_field_names": ["PID"], "excludes": [1], "wf_analysis": True}
    # otherwise: evaluation_config first, the calibration with setdefault
    monkeypatch.setattr(litz, "calibration_from_config", lambda config: {"calibration": "CURVES", "n_samples": 20})
    m, ev = _evaluator_of("LitZ", recorded, "ZEvaluator", evaluation_config={"n_samples": 99, "nmult": 3})
    assert not m.test_has_phys and ev.args == (CPU,)
    assert ev.kwargs == {"n_samples": 99, "nmult": 3, "calibration": "CURVES"}
    _, ev = _evaluator_of("LitZ", recorded, "ZEvaluator")
    assert ev.kwargs == {"calibration": "CURVES", "n_samples": 20}


def test_litez_evaluator_keywords(recorded, monkeypatch):
    from waveformml_amd.psd import litz
    # E_scale = e_adjust with setdefault, before the calibration
    _, ev = _evaluator_of("LitEZ", recorded, "EZEvaluator", net_config={"e_adjust": 6.0})
    assert ev.args == (CPU,) and ev.kwargs == {"E_scale": 6.0}
    monkeypatch.setattr(litz, "calibration_from_config", lambda config: {"calibration": "CURVES", "E_scale": 1.0, "n_samples": 20})
    _, ev = _evaluator_of("LitEZ", recorded, "EZEvaluator", net_config={"e_adjust": 6.0},
                          evaluation_config={"E_scale": 2.0, "n_samples": 99})
    assert ev.kwargs == {"E_scale": 2.0, "n_samples": 99, "calibration": "CURVES"}
    _, ev = _evaluator_of("LitEZ", recorded, "EZEvaluator", net_config={"e_adjust": 6.0})
    assert ev.kwargs == {"E_scale": 6.0, "calibration": "CURVES", "n_samples": 20}


def test_litwaveform_evaluator_keywords(recorded):
    _, ev = _evaluator_of("LitWaveform", recorded, "TensorEvaluator", evaluation_config={"metric_unit": "mm"})
    assert ev.args == (CPU,)
    assert ev.kwargs == {"calgroup": None, "target_has_phys": False, "target_index": 7,
                         "metric_name": "mean absolute error", "metric_unit": "mm"}
    m, ev = _evaluator_of("LitWaveform", recorded, "TensorEvaluator", dataset_config=dict(FIELDS, calgroup="Cal"))
    assert m.test_has_phys and ev.kwargs == {"calgroup": "Cal", "target_has_phys": True, "target_index": 7,
                                             "metric_name": "mean absolute error"}
    # a key of evaluation_config that repeats one of the four explicit keywords
    m = lc.build("LitWaveform", lambda cfg: cfg.update(evaluation_config={"metric_name": "x"}))
    with pytest.raises(TypeError, match="multiple values for keyword argument 'metric_name'"):
        m.evaluator


def test_litpsd_evaluator_choice(recorded):
    names = ["Gamma", "Electron", "Positron"]
    _, ev = _evaluator_of("LitPSD", recorded, "PSDEvaluator", evaluation_config={"n_bins": 5})
    assert ev.args == (names, CPU) and ev.kwargs == {"n_samples": 150}               # evaluation_config is not read
    _, ev = _evaluator_of("LitPSD", recorded, "PhysEvaluator", dataset_config={"dataset_class": "PulseDataset.PulseDatasetDet"},
                          evaluation_config={"n_bins": 5, "emax": 3.0})
    assert ev.args == (names, CPU) and ev.kwargs == {"n_bins": 5, "emax": 3.0}
    # no type names: None, and asked for again on the next read
    Recorder.made = []
    m = lc.build("LitPSD", lambda cfg: cfg["system_config"].pop("type_names"))
    assert m.evaluator is None and m.evaluator is None and Recorder.made == []
    m.config.system_config.type_names = names
    assert type(m.evaluator) is recorded["PSDEvaluator"]


SCHEDULER_ERROR = ("Optimizer config has a learning scheduler class specified. You must also set lr_schedule_parameters "
                   "(dictionary of key value pairs).")


def _with_scheduler(params):
    def edit(cfg):
        oc = cfg["optimize_config"]
        oc["imports"] = ["torch.optim", "torch.optim.lr_scheduler"]
        oc["scheduler_class"] = "lr_scheduler.ExponentialLR"
        oc.pop("scheduler_params", None)
        if params is not None:
            oc["scheduler_params"] = params
    return edit


@pytest.mark.parametrize("name", ["LitPSD", "LitZ"])
def test_optimizer_with_a_flat_parameter_set(name):
    """``Trainer.fit`` sets ``optimizer_parameters`` on every module: LitPSD optimises that tensor, single-tensor kernels
    (``foreach=False``); LitZ (and LitEZ, the same base) goes on optimising ``model.parameters()``."""
    m = lc.build(name, _with_scheduler({"gamma": 0.9}))
    flat = torch.zeros(sum(p.numel() for p in m.model.parameters()), requires_grad=True)
    m.optimizer_parameters = [flat]
    (opt,), (sched,) = m.configure_optimizers()
    assert type(opt) is torch.optim.SGD and type(sched).__name__ == "ExponentialLR" and sched.optimizer is opt
    assert opt.defaults["lr"] == m.lr and opt.defaults["momentum"] == m.config.optimize_config.optimizer_params.momentum
    got = [p for g in opt.param_groups for p in g["params"]]
    if name == "LitPSD":
        assert len(got) == 1 and got[0] is flat and opt.defaults["foreach"] is False
    else:
        model = list(m.model.parameters())
        assert len(got) == len(model) and all(a is b for a, b in zip(got, model)) and opt.defaults["foreach"] is None
    # no scheduler class: the bare optimizer; a class without parameters: the reference's error
    m.config.optimize_config.scheduler_class = None
    assert type(m.configure_optimizers()) is torch.optim.SGD
    bad = lc.build(name, _with_scheduler(None))
    bad.optimizer_parameters = [flat]
    with pytest.raises(IOError) as err:
        bad.configure_optimizers()
    assert str(err.value) == SCHEDULER_ERROR


def test_litz_names_the_padded_batch_it_does_not_take():
    m = _module("LitZ")
    c = torch.tensor([[1, 2, 0], [3, 4, 0]], dtype=torch.int32)
    batch = ([c, torch.rand(2, 40), torch.tensor([2])], torch.rand(2))
    with pytest.raises(ValueError, match="do not take a capacity-padded batch"):
        m.training_step(batch, 0)
