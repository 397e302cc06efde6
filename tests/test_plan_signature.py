"""Every plan the engine builds is launch for launch the one recorded in tests/golden/plan_signatures.json
(tools/plan_signature.py: the canonical, address-free text of a launch list; the file keeps its sha256 and
launch count per configuration).  The file is the yardstick for a rewrite of the planner: it is recorded from
the planner as it stands and never regenerated from the code under test.  Where an entry differs the planner
moved a launch, and `python tools/plan_signature.py --dump CONFIG` on both revisions shows which."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, REPO

_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(REPO, "tools", "plan_signature.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

with open(os.path.join(GOLDEN, "plan_signatures.json")) as _fh:
    RECORDED = json.load(_fh)

HOST = S.host_configs()


def _check(name, spec):
    recorded = RECORDED[S.setting()]
    for suffix, text in S.signatures_of(spec).items():
        assert name + suffix in recorded, f"{name + suffix} is not recorded"
        assert S.digest(text) == recorded[name + suffix], name + suffix


@pytest.mark.parametrize("name", list(HOST))
def test_host_plan_matches_recorded_signature(name):
    """device="cpu", fp32 packed weights: builds without a GPU (the library's tile rules still read the CU
    count where there is one, so the entries are keyed by whether a GPU is present)."""
    _check(name, HOST[name])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", S.GPU_PRECISIONS)
def test_gpu_plans_match_recorded_signatures(prec):
    """The pair / stream / bidi rows on the device: raft_corr_lookup_conv, the in-loader InstanceNorm and (f16x3)
    the range-flag pointers, each of which signatures_of asserts to be the plan's own range_flag.  Plans are
    only built; no forward runs."""
    for name, spec in S.gpu_configs((prec,)).items():
        _check(name, spec)


def test_recorded_file_covers_the_matrix():
    for key in ("none", "gpu"):
        missing = [n for n in HOST if n not in RECORDED[key]]
        assert not missing, (key, missing)
    assert all(n in RECORDED["gpu"] for n in S.gpu_configs())
