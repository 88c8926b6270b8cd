"""GPU: the bindings reach the library through rrnet_amd._C.call — a launch through it computes what it did, and a wrapper
that never had a device check of its own (ops.dcn_fwd) now refuses a host tensor before any entry point is fetched."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_relu_fwd_through_call_equals_torch_relu():
    from rrnet_amd import ops
    g = torch.Generator().manual_seed(7)
    x = ops.to_nhwc(torch.randn(1, 4, 2, 2, generator=g).cuda())
    assert torch.equal(ops.relu_fwd(x), torch.relu(x))


def test_dcn_fwd_refuses_a_host_offset_before_any_entry_is_reached(monkeypatch):
    from rrnet_amd import _C, ops

    def no_entry(name, *a, **kw):
        raise AssertionError("%s was looked up" % name)

    x = ops.to_nhwc(torch.zeros(1, 4, 4, 4).cuda())
    w = ops.to_nhwc(torch.zeros(4, 4, 3, 3).cuda())
    offset, mask = ops.to_nhwc(torch.zeros(1, 18, 4, 4)), ops.to_nhwc(torch.zeros(1, 9, 4, 4).cuda())
    monkeypatch.setattr(_C, "fn", no_entry)                 # whichever way the test goes, nothing is launched
    with pytest.raises(_C.RRNetHipError, match="MI355X only: got a cpu tensor"):
        ops.dcn_fwd(x, offset, mask, w, None, 1, (1, 1), 1, 1)
