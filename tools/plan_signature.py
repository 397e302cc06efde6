#!/usr/bin/env python3
"""Address-free signatures of the engine's launch plans.

A plan is a fixed list of C-ABI launches with raw pointers.  This tool builds plans for a matrix of
configurations and reduces each launch list to a canonical text that does not depend on where the
allocator put the buffers, so that two revisions of the planner can be compared launch for launch:

  fork / join            the markers, as they are
  NAME side=S ARGS...    one Launch; every pointer argument (the library function's ctypes argtypes
                         say which) is written tK+OFF: K numbers the tensors (storages) in order of
                         first appearance in the list, OFF is the byte offset into that storage.
                         Structures (ConvParams behind byref, Copy2D) and ctypes arrays are walked
                         field by field under the same rule; everything else is written by value.

A pointer that lies in no tensor reachable from the plan is an error.

  python tools/plan_signature.py --write tests/golden/plan_signatures.json
  python tools/plan_signature.py --check tests/golden/plan_signatures.json
  python tools/plan_signature.py --dump pair/full/allpairs/test

The recorded file keeps a sha256 of each text and its launch count, under the key `none` or `gpu`
(torch.cuda.is_available(): the library's tile rules read the device's CU count).  The host matrix
(device="cpu", fp32 weights) is part of both; with a GPU the pair / stream / bidi rows are repeated on
the device in f16x3, f16 and bf16.  --write replaces the entries of the setting it runs under and keeps
the other's.
"""
from __future__ import annotations

import argparse
import bisect
import contextlib
import ctypes
import functools
import hashlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from raft_optical_flow_amd import _lib  # noqa: E402
from raft_optical_flow_amd import engine as E  # noqa: E402
from raft_optical_flow_amd import kernels as K  # noqa: E402

# the plan-time switches, each with the values the matrix moves it to
SWITCHES = [("RAFT_CTX_SIDE", "0"), ("RAFT_FLOW_SIDE", "0"), ("RAFT_CONV_PAIR", "0"), ("RAFT_FUSE_CONVF1", "0"),
            ("RAFT_FUSE_CONVC1", "0"), ("RAFT_EPI_STATS", "0"), ("RAFT_IN_NORM", "0"), ("RAFT_MERGE_FUSED", "0"),
            ("RAFT_CTX_ORDER", "early"), ("RAFT_CTX_ORDER", "mix")]
GPU_PRECISIONS = ("f16x3", "f16", "bf16")
PAIR_HW = (128, 192)
FRAME_HW = (123, 181)     # pads by 1, 2, 2, 3 to 128 x 184: non-zero crop offsets
BLOCK_NHW = (2, 16, 24)
ITERS = 2

# the range-flag arguments of the launches that take one outside a ConvParams (include/raft_hip.h)
FLAG_ARGS = {"raft_corr_lookup": (13,), "raft_corr_lookup_convf1": (13, 21), "raft_corr_lookup_conv": (9, 16, 23),
             "raft_alt_corr_lookup_levels_prec": (17,), "raft_convf1_flow": (12,)}


def setting() -> str:
    return "gpu" if torch.cuda.is_available() else "none"


# ----------------------------------------------------------------------------
# Launch list -> canonical text
# ----------------------------------------------------------------------------


def tensors_of(obj, out=None, _seen=None):
    """Every tensor reachable from obj (attributes, slots of Launch / Rows, lists, tuples, dicts): the
    same kind of walk as kernels.set_precision."""
    out = [] if out is None else out
    _seen = set() if _seen is None else _seen
    if obj is None or isinstance(obj, (int, float, str, bytes, type, types.ModuleType, ctypes.Structure,
                                       ctypes.Array)) or id(obj) in _seen:
        return out
    _seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        out.append(obj)
        return out
    if isinstance(obj, (list, tuple, set)):
        items = list(obj)
    elif isinstance(obj, dict):
        items = list(obj.values())
    elif isinstance(obj, K.Launch):
        items = [obj.keep]
    elif isinstance(obj, K.Rows):
        items = [obj.t]
    elif hasattr(obj, "__dict__"):
        items = list(vars(obj).values())
    else:
        return out
    for v in items:
        tensors_of(v, out, _seen)
    return out


class _Canon:
    """Pointer -> (tensor number, byte offset) over the storages of a set of tensors."""

    def __init__(self, tensors):
        spans = {}
        for t in tensors:
            s = t.untyped_storage()
            if s.nbytes() > 0:
                spans[s.data_ptr()] = max(spans.get(s.data_ptr(), 0), s.nbytes())
        self.starts = sorted(spans)
        self.sizes = [spans[a] for a in self.starts]
        self.number = {}
        self.flags = []   # raw values of the non-null range-flag pointers met

    def ptr(self, v, what):
        if v is None:
            return "None"
        i = bisect.bisect_right(self.starts, v) - 1
        if i < 0 or v >= self.starts[i] + self.sizes[i]:
            raise LookupError(f"{what}: pointer {v:#x} lies in no tensor reachable from the plan")
        k = self.number.setdefault(self.starts[i], len(self.number))
        return f"t{k}+{v - self.starts[i]}"

    def value(self, v, ctype, what):
        if isinstance(v, ctypes.Array):
            return "[" + ",".join(self.value(e, v._type_, f"{what}[{i}]") for i, e in enumerate(v)) + "]"
        if isinstance(v, ctypes.Structure):
            return self.struct(v, what)
        if hasattr(v, "_obj"):    # ctypes.byref(x)
            return self.value(v._obj, type(v._obj), what)
        if ctype is ctypes.c_void_p:
            return self.ptr(v, what)
        if isinstance(v, ctypes._SimpleCData):
            v = v.value
        return repr(float(v)) if ctype is ctypes.c_float else repr(v)

    def struct(self, s, what):
        parts = []
        for name, ftype in s._fields_:
            v = getattr(s, name)
            if isinstance(s, _lib.ConvParams) and name == "range_flag" and v is not None:
                self.flags.append(v)
            parts.append(f"{name}={self.value(v, ftype, f'{what}.{name}')}")
        return "{" + ",".join(parts) + "}"

    def launch(self, l):
        argtypes = l.fn.argtypes
        assert len(argtypes) == len(l.args) + 1, (l.name, len(argtypes), len(l.args))   # + the stream
        for i in FLAG_ARGS.get(l.name, ()):
            if l.args[i] is not None:
                self.flags.append(l.args[i])
        args = [self.value(a, t, f"{l.name} arg {i}") for i, (a, t) in enumerate(zip(l.args, argtypes))]
        return f"{l.name} side={int(bool(l.side))} " + " ".join(args)


def signature(launches, roots):
    """(canonical text, the raw range-flag pointers in it) of a launch list whose buffers are reachable
    from `roots` (any objects) or from a Launch.keep."""
    canon = _Canon(tensors_of([roots, launches]))
    lines = [l if isinstance(l, str) else canon.launch(l) for l in launches]
    return "\n".join(lines) + "\n", canon.flags


def digest(text: str) -> dict:
    return {"sha256": hashlib.sha256(text.encode()).hexdigest(),
            "launches": sum(1 for ln in text.splitlines() if ln not in (K.FORK, K.JOIN))}


# ----------------------------------------------------------------------------
# The configurations
# ----------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def packed(small: bool, device: str, prec: str):
    """PackedRaft of a freshly initialised model (the values do not enter a signature)."""
    import argparse as ap

    from raft_optical_flow_amd import RAFT
    model = RAFT(ap.Namespace(small=small, mixed_precision=False, alternate_corr=False)).eval()
    with torch.no_grad():
        return E.PackedRaft(model, device, _lib.PRECISIONS[prec])


def _plan_rows(prefix, device, prec):
    rows = {}
    for net in ("full", "small"):
        for corr in ("allpairs", "alt"):
            base = dict(small=net == "small", alternate=corr == "alt", device=device, prec=prec)
            rows[f"{prefix}pair/{net}/{corr}/test"] = dict(base, kind="pair", kw=dict(test_mode=True))
            rows[f"{prefix}pair/{net}/{corr}/iters+init"] = dict(base, kind="pair",
                                                                 kw=dict(test_mode=False, flow_init=True))
            rows[f"{prefix}stream/{net}/{corr}/warm"] = dict(base, kind="stream", kw=dict(warm_start=True))
            rows[f"{prefix}bidi/{net}/{corr}/warm"] = dict(base, kind="bidi", kw=dict(warm_start=True))
    rows[f"{prefix}stream/full/allpairs/warm+viz"] = dict(
        small=False, alternate=False, device=device, prec=prec, kind="stream",
        kw=dict(warm_start=True, visualize="rgb", viz_stack=True))
    return rows


def host_configs() -> dict:
    """name -> spec of the host matrix (device="cpu", fp32 packed weights: no kernel runs)."""
    rows = _plan_rows("", "cpu", "fp32")
    for env, val in SWITCHES:
        rows[f"pair/full/allpairs/test/{env}={val}"] = dict(rows["pair/full/allpairs/test"], env={env: val})
    rows["pair/small/allpairs/test/RAFT_FLOW_SIDE=0"] = dict(rows["pair/small/allpairs/test"],
                                                             env={"RAFT_FLOW_SIDE": "0"})
    for block in ("residual", "bottleneck"):
        for norm in ("group", "instance", "batch", "none"):
            for stride in (1, 2):
                rows[f"block/{block}/{norm}/s{stride}"] = dict(kind="block", block=block, norm=norm, stride=stride)
    for net in ("full", "small"):
        rows[f"update/{net}"] = dict(kind="update", small=net == "small")
    return rows


def gpu_configs(precisions=GPU_PRECISIONS) -> dict:
    """The pair / stream / bidi rows on the device, per conv precision."""
    rows = {}
    for prec in precisions:
        rows.update(_plan_rows(f"gpu/{prec}/", "cuda", prec))
    return rows


def all_configs() -> dict:
    rows = host_configs()
    if torch.cuda.is_available():
        rows.update(gpu_configs())
    return rows


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _build_block(spec):
    from raft_optical_flow_amd.extractor import BottleneckBlock, ResidualBlock
    small = spec["block"] == "bottleneck"
    n, h, w = BLOCK_NHW
    cin, planes = (64, 64) if spec["stride"] == 1 else (64, 96)
    blk = (BottleneckBlock if small else ResidualBlock)(cin, planes, spec["norm"], stride=spec["stride"]).eval()
    with torch.no_grad():
        d = E.pack_block(blk, spec["norm"], small, "cpu")
    pe = types.SimpleNamespace(norm=spec["norm"], small=small)
    L, A = [], E.Arena("cpu")
    xr = K.Rows(A.rows(n * h * w, cin))
    (E._plan_bottleneck if small else E._plan_residual)(L, A, pe, d, xr, n, h, w)
    return L, (A, d, xr)


def _build_update(spec):
    """plan_gru_context + plan_update as update._UpdateBase.forward calls them."""
    import argparse as ap

    from raft_optical_flow_amd.update import BasicUpdateBlock, SmallUpdateBlock
    small = spec["small"]
    args = ap.Namespace(corr_levels=4, corr_radius=3 if small else 4)
    mod = (SmallUpdateBlock(args, hidden_dim=96) if small else BasicUpdateBlock(args, hidden_dim=128)).eval()
    b, h, w = 1, BLOCK_NHW[1], BLOCK_NHW[2]
    with torch.no_grad():
        pu = E.PackedUpdate(mod, small, "cpu")
    A = E.Arena("cpu")
    ub = E.UpdateBuffers(A, pu, b * h * w, pu.cor_planes)
    L = []
    E.plan_gru_context(L, pu, ub, b, h, w)
    E.plan_update(L, pu, ub, b, h, w, with_mask=not small)
    return L, (A, ub, pu)


def signatures_of(spec, **plan_kw) -> dict:
    """{"": text of the launch list, "#prime": text of the prime list where the plan has one} of one
    configuration.  plan_kw goes to the plan's constructor (pair / stream / bidi rows)."""
    with _environ(spec.get("env", {})):
        if spec["kind"] == "block":
            return {"": signature(*_build_block(spec))[0]}
        if spec["kind"] == "update":
            return {"": signature(*_build_update(spec))[0]}
        pk = packed(spec["small"], spec["device"], spec["prec"])
        kw = dict(spec["kw"], alternate=spec["alternate"], device=spec["device"], **plan_kw)
        if spec["kind"] == "pair":
            plan = E.RaftPlan(pk, 1, *PAIR_HW, ITERS, **kw)
        else:
            plan = (E.StreamPlan if spec["kind"] == "stream" else E.BidiStreamPlan)(pk, 1, *FRAME_HW, ITERS, **kw)
    try:
        text, flags = signature(plan.launches, plan)
        out = {"": text}
        if getattr(plan, "prime_launches", None):
            prime, pflags = signature(plan.prime_launches, plan)
            out["#prime"] = prime
            flags = flags + pflags
        if spec["device"] != "cpu" and spec["prec"] == "f16x3":
            # the guard is on: every range flag in the lists is this plan's own
            assert plan.guarded and flags, (plan.guarded, len(flags))
            own = plan.range_flag.data_ptr()
            assert all(f == own for f in flags), "a range-flag pointer is not the plan's own range_flag"
        else:
            assert not flags, "range-flag pointers in a plan without the f16x3 guard"
        return out
    finally:
        plan.release()


def compute(configs: dict) -> dict:
    out = {}
    for name, spec in configs.items():
        for suffix, text in signatures_of(spec).items():
            out[name + suffix] = digest(text)
    return out


def check(recorded: dict, configs: dict) -> list:
    """Names of the configurations whose signature differs from the recorded one."""
    got = compute(configs)
    return [n for n in got if recorded.get(n) != got[n]]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", metavar="FILE", help="record the signatures of this setting into FILE")
    g.add_argument("--check", metavar="FILE", help="compare against FILE; exit 1 where an entry differs")
    g.add_argument("--dump", metavar="CONFIG", help="print one configuration's signature, one launch per line")
    a = ap.parse_args(argv)
    configs = all_configs()
    if a.dump:
        if a.dump not in configs:
            ap.error(f"unknown configuration {a.dump!r}; known:\n  " + "\n  ".join(configs))
        for suffix, text in signatures_of(configs[a.dump]).items():
            print(f"== {a.dump}{suffix}")
            sys.stdout.write(text)
        return 0
    if a.write:
        data = {}
        if os.path.exists(a.write):
            with open(a.write) as fh:
                data = json.load(fh)
        data[setting()] = compute(configs)
        with open(a.write, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print(f"{a.write}: {len(data[setting()])} signatures under {setting()!r}")
        return 0
    with open(a.check) as fh:
        recorded = json.load(fh).get(setting())
    if recorded is None:
        print(f"{a.check} has no entries for the setting {setting()!r}")
        return 1
    bad = check(recorded, configs)
    for n in bad:
        print(f"DIFFERS: {n}")
    print(f"{len(configs)} configurations, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
