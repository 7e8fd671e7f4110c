"""The per-layer store of sticky flags and build state (spconv.ops._sticky_flags) on CPU tensors: one tensor per (name,
size), created once and handed back to every later build, ``store[name]`` the latest one handed out.  A build for
another size (the event-local conv build's look-back state grows past 512 events) must not replace the tensor a
captured graph of the first size still writes."""
import torch

from waveformml_amd.spconv import ops


def test_store_is_keyed_by_name_and_size():
    cpu = torch.device("cpu")
    store = {}
    a = ops._sticky_flags(8, cpu, store, "conv_state")
    assert a.dtype == torch.int32 and a.numel() == 8 and not a.any()
    a[0] = 5
    assert ops._sticky_flags(8, cpu, store, "conv_state") is a           # the same tensor for the same size
    assert store["conv_state"] is a                                       # the latest build's, by name
    b = ops._sticky_flags(12, cpu, store, "conv_state")                   # another size: its own tensor ...
    assert b is not a and b.numel() == 12 and not b.any()
    assert store["conv_state"] is b and store[("conv_state", 8)] is a     # ... and the first one is still held
    assert ops._sticky_flags(8, cpu, store, "conv_state") is a
    assert int(a[0]) == 5 and store["conv_state"] is a
    assert ops._sticky_flags(12, cpu, store, "conv_state") is b
    c = ops._sticky_flags(8, cpu, store, "overflow")                      # names never share a tensor
    assert c is not a and not c.any()
    assert set(store) == {"conv_state", ("conv_state", 8), ("conv_state", 12), "overflow", ("overflow", 8)}


def test_without_a_store_every_call_gets_fresh_zeros():
    cpu = torch.device("cpu")
    a = ops._sticky_flags(4, cpu)
    a[:] = 1
    b = ops._sticky_flags(4, cpu)
    assert b is not a and not b.any()
