"""RAFT._plan_key names every variable that is read while a plan is built, so a forward under one setting
never reuses the plan built under another (no GPU: the key is host arithmetic, the plans are the device="cpu"
ones of tools/plan_signature.py)."""
import argparse
import importlib.util
import os
import re

import pytest

from conftest import REPO
from raft_optical_flow_amd import RAFT

_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(REPO, "tools", "plan_signature.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

# read once when a model is constructed: attributes of the model, not of a plan
LOAD_TIME = {"RAFT_HIP_GRAPH", "RAFT_MAX_PLANS", "RAFT_RANGE_GUARD"}
KEY_ARGS = (1, 128, 192, 2, True, False, "fp32")


@pytest.fixture(scope="module")
def model():
    return RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).eval()


@pytest.fixture
def clean_env(monkeypatch):
    for name in {n for n, _ in S.SWITCHES}:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("name,value", S.SWITCHES, ids=[f"{n}={v}" for n, v in S.SWITCHES])
def test_plan_key_moves_with_every_switch(model, clean_env, name, value):
    default = model._plan_key(*KEY_ARGS)
    assert model._plan_key(*KEY_ARGS) == default
    clean_env.setenv(name, value)
    assert model._plan_key(*KEY_ARGS) != default, f"{name}={value}: a forward would reuse the default plan"


def test_the_two_ctx_orders_have_keys_of_their_own(model, clean_env):
    keys = set()
    for v in ("late", "early", "mix"):
        clean_env.setenv("RAFT_CTX_ORDER", v)
        keys.add(model._plan_key(*KEY_ARGS))
    assert len(keys) == 3


def _env_reads(path):
    with open(path) as fh:
        src = fh.read()
    return set(re.findall(r"os\.environ\.get\(\s*[\"'](RAFT_[A-Z0-9_]+)[\"']", src)), src


def test_plan_key_names_every_plan_time_variable():
    pkg = os.path.join(REPO, "raft_optical_flow_amd")
    eng, _ = _env_reads(os.path.join(pkg, "engine.py"))
    rft, src = _env_reads(os.path.join(pkg, "raft.py"))
    assert eng, "the regex found no os.environ.get(\"RAFT_...\") in engine.py"
    body = src[src.index("def _plan_key"):]
    body = body[:body.index("\n    def ", 1)]
    in_key = set(re.findall(r"os\.environ\.get\(\s*[\"'](RAFT_[A-Z0-9_]+)[\"']", body))
    plan_time = (eng | rft) - LOAD_TIME
    assert plan_time - in_key == set(), f"read while a plan is built but not in _plan_key: {sorted(plan_time - in_key)}"
    assert in_key - plan_time == set(), sorted(in_key - plan_time)
    # the signature matrix moves exactly these
    assert {n for n, _ in S.SWITCHES} == plan_time


@pytest.mark.parametrize("name,value", [s for s in S.SWITCHES if s[0] in ("RAFT_MERGE_FUSED", "RAFT_CTX_ORDER")],
                         ids=lambda v: str(v))
def test_the_added_knobs_do_change_the_plan(name, value):
    """RAFT_MERGE_FUSED and RAFT_CTX_ORDER are plan-time: the device="cpu" launch list differs from the default's."""
    host = S.host_configs()
    base = S.signatures_of(host["pair/full/allpairs/test"])[""]
    assert S.signatures_of(host[f"pair/full/allpairs/test/{name}={value}"])[""] != base
