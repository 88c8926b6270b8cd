"""GPU: the backward convolution dispatch of rrnet_amd/ops.py (dgrad_route -> conv_dgrad's launchers, conv_wgrad) pinned at the
ABI.  tests/golden/conv_bwd_routes.json holds, for every call of tests/conv_route_cases.py, what reached the library — entry
points with their non-pointer arguments, timer names, FLOPs and byte counts — recorded on an MI355X from the dispatch as it
stood before dgrad_route existed (the nested conditions of the parent commit).  The same calls must produce the same launches."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ENTRY_POINTS = ["rr_conv16_dgrad_s1_relumask", "rr_head_dgrad_relubias",
                "rr_conv_dgrad_s1_relubias", "rr_conv_dgrad_s1_relubias_bf16", "rr_conv_dgrad_s1_relubias_f16x3",
                "rr_conv16_dgrad_s1", "rr_conv_dgrad_s1_bnsum", "rr_conv_dgrad_s1_bnsum_bf16", "rr_conv_dgrad_s1_bnsum_f16x3",
                "rr_conv_dgrad_s1", "rr_conv_dgrad_s1_bf16", "rr_conv_dgrad_s1_f16x3", "rr_conv16_dgrad_s2",
                "rr_conv_dgrad_s2_bf16", "rr_conv_dgrad_s2_f16x3", "rr_conv_dgrad", "rr_conv16_wgrad",
                "rr_conv_wgrad", "rr_conv_wgrad_bf16", "rr_conv_wgrad_f16x3"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "conv_bwd_routes.json")) as fh:
        return json.load(fh)


def test_golden_holds_every_case_and_reaches_every_backward_entry_point(golden):
    """A condition on the FIXTURE: a golden that quietly lost a route (or a case) fails here."""
    from conv_route_cases import cases
    assert list(golden) == [c["id"] for c in cases()]
    called = {e[1] for rec in golden.values() for e in rec if e[0] == "C"}
    assert not [n for n in ENTRY_POINTS if n not in called], [n for n in ENTRY_POINTS if n not in called]
    widening = [c["id"] for c in cases() if c["b16"] and any(e[1] == "rr_from_bf16" for e in golden[c["id"]])]
    assert widening, "no case with a bf16-only operand records rr_from_bf16"
    assert all(rec and rec[-1][0] == "C" for rec in golden.values())          # every case ends in its convolution launch


def test_backward_convolution_launches_equal_the_golden(golden):
    from rrnet_amd import ops
    from conv_route_cases import record
    got = json.loads(json.dumps(record(ops)))
    assert list(got) == list(golden)
    for cid, want in golden.items():
        assert got[cid] == want, "first differing case %s\n golden: %s\n    now: %s" % (cid, want, got[cid])
