#!/usr/bin/env python3
"""Signatures of the conv dispatch: what the library's host code decides for a conv, case by case.

raft_conv2d picks a kernel and an instantiation for every conv (halo tile rows and columns, tiles per
work-group, loader waves, compute waves per SIMD; the GEMM kernel's K-groups; the small-N tile rows), and the
planner sizes buffers from the queries beside it.  This tool asks every host-side query about a list of convs,
with stand-in pointers and nothing launched, and writes one text line per conv:

  NAME rc=R form=k,rows,cols,m,nl,ks,kg,sn slots=S rows=T m=M norm=N | pair(NEXT) rc=R one=O f0=... f1=...

  rc, form   raft_conv2d_form of the conv with its features (stats_part / in_norm) set
  slots      raft_conv2d_stats_slots, asked with stats_part unset (as the planner asks, before it sets it)
  rows, m    raft_conv2d_halo_tile_rows, raft_conv2d_halo_tiles_per_wg
  norm       raft_conv2d_in_norm_ok
  pair       raft_conv2d_pair_form of the bare conv and the next case of the same B, H, W (independent operands)

The cases: conv_forms.TABLE and ENC_TABLE, the update-block and encoder convs of RAFT-full and RAFT-small at five
workload sizes, and 2000 seeded random shapes.  The settings: the default and every dispatch knob moved off its
default, one at a time, each in a fresh child process (most knobs are cached for the life of a process).

  python tools/conv_dispatch_signature.py --write tests/golden/conv_dispatch_signatures.json
  python tools/conv_dispatch_signature.py --check tests/golden/conv_dispatch_signatures.json
  python tools/conv_dispatch_signature.py --dump RAFT_HALO_MT=0        (or: default)

The recorded file keeps a sha256 and a line count per setting.  It is the yardstick for a rewrite of the dispatch:
recorded from the library as it stood before, never from the code under test.  Without a device the library
assumes 256 CUs, MI355X's count, so one file holds with and without a GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

if "--child" in sys.argv[1:] and "raft_optical_flow_amd" not in sys.modules:
    # a child needs the ctypes binding alone: name the package without running its __init__ (which imports torch,
    # most of a child's run time otherwise)
    import types
    _pkg = types.ModuleType("raft_optical_flow_amd")
    _pkg.__path__ = [os.path.join(ROOT, "raft_optical_flow_amd")]
    sys.modules["raft_optical_flow_amd"] = _pkg

from raft_optical_flow_amd import _lib  # noqa: E402

import conv_forms as CF  # noqa: E402

SETTINGS = ["default", "RAFT_CONV_HALO=0", "RAFT_CONV_STEM=0", "RAFT_HALO_NL8=0", "RAFT_HALO_KS2=0",
            "RAFT_HALO_NL8_ENC=0", "RAFT_HALO_MT=0", "RAFT_HALO_BIG_MIN=0", "RAFT_HALO_BIG_MT=1", "RAFT_HALO_WIDE=0",
            "RAFT_HALO_WIDE_MIN=512", "RAFT_HALO_MT_COST=0.5", "RAFT_HALO_BIG_COST=1.5", "RAFT_GEMM_STATS=0",
            "RAFT_SN_TH4_MIN=1"]
KNOBS = sorted({s.split("=")[0] for s in SETTINGS[1:]})
CHILD_TIMEOUT = 120   # seconds per setting
WORKLOADS = ((1, 128, 192), (1, 440, 1024), (2, 436, 1024), (1, 1080, 1920), (8, 135, 240))
PRECS = ("fp32", "f16x3", "bf16", "f16")
N_RANDOM, SEED = 2000, 20240229
RANDOM_N = (1, 2, 3, 4, 32, 64, 96, 100, 126, 128, 192, 256, 384, 512, 576)
RANDOM_K = ((1, 1), (3, 3), (1, 5), (5, 1), (7, 7))

# a conv and how it is asked about: conv_forms' shape fields, the epilogue, whether an f16x3 conv carries the scaled
# weight, and the features to set where the shape allows them
Case = namedtuple("Case", "name B H W cin n kh kw stride prec epilogue scaled stats in_norm")


def _case(name, B, H, W, cin, n, k, stride, prec, epilogue=_lib.EPI_LINEAR, scaled=True, stats=False, in_norm=False):
    return Case(name, B, H, W, cin, n, k[0], k[1], stride, prec, epilogue, scaled, stats, in_norm)


def _table_cases():
    out = []
    for c in CF.TABLE:
        out.append(_case("table/" + c.name, c.B, c.H, c.W, c.cin, c.n, (c.kh, c.kw), c.stride, c.prec))
    for c in CF.ENC_TABLE:
        out.append(_case("enc/" + c.name, c.B, c.H, c.W, c.cin, c.n, (c.kh, c.kw), c.stride, c.prec,
                         stats=c.stats, in_norm=c.in_norm))
    return out


def _encoder(small):
    """(name, cin, n, k, stride, downscale of the input) of one encoder's convs."""
    if not small:
        convs = [("stem", 3, 64, 7, 2, 1)]
        convs += [(f"l1.{i}", 64, 64, 3, 1, 2) for i in range(4)]
        convs += [("l2.0", 64, 96, 3, 2, 2), ("l2.down", 64, 96, 1, 2, 2)] + [(f"l2.{i}", 96, 96, 3, 1, 4) for i in (1, 2, 3)]
        convs += [("l3.0", 96, 128, 3, 2, 4), ("l3.down", 96, 128, 1, 2, 4)]
        convs += [(f"l3.{i}", 128, 128, 3, 1, 8) for i in (1, 2, 3)] + [("out", 128, 256, 1, 1, 8)]
        return convs
    convs = [("stem", 3, 32, 7, 2, 1)]
    for name, cin, planes, stride, ds in (("l1.0", 32, 32, 1, 2), ("l1.1", 32, 32, 1, 2), ("l2.0", 32, 64, 2, 2),
                                          ("l2.1", 64, 64, 1, 4), ("l3.0", 64, 96, 2, 4), ("l3.1", 96, 96, 1, 8)):
        q = planes // 4
        convs += [(name + ".a", cin, q, 1, 1, ds), (name + ".b", q, q, 3, stride, ds), (name + ".c", q, planes, 1, 1, ds * stride)]
        if stride == 2:
            convs.append((name + ".down", cin, planes, 1, 2, ds))
    convs += [("out-f", 96, 128, 1, 1, 8), ("out-c", 96, 160, 1, 1, 8)]
    return convs


def _update(small):
    """(name, cin, n, (kh, kw)) of the update block's convs at 1/8 resolution (the GRU's z | r convs as one)."""
    if not small:
        return [("convc1", 324, 256, (1, 1)), ("convc2", 256, 192, (3, 3)), ("convf1", 2, 128, (7, 7)),
                ("convf2", 128, 64, (3, 3)), ("conv", 256, 126, (3, 3)), ("zr1", 384, 256, (1, 5)),
                ("q1", 384, 128, (1, 5)), ("zr2", 384, 256, (5, 1)), ("q2", 384, 128, (5, 1)),
                ("fh1", 128, 256, (3, 3)), ("fh2", 256, 2, (3, 3)), ("mask1", 128, 256, (3, 3)),
                ("mask2", 256, 576, (1, 1))]
    return [("convc1", 196, 96, (1, 1)), ("convf1", 2, 64, (7, 7)), ("convf2", 64, 32, (3, 3)),
            ("conv", 128, 80, (3, 3)), ("zr", 244, 192, (3, 3)), ("q", 244, 96, (3, 3)), ("fh1", 96, 128, (3, 3)),
            ("fh2", 128, 2, (3, 3))]


def _down(x, ds):
    """x after the stride-2 convs ahead of a 1/ds-resolution layer (7x7 pad 3 and 3x3 pad 1 both halve rounding up)."""
    while ds > 1:
        x, ds = (x + 1) // 2, ds // 2
    return x


def _workload_cases():
    out = []
    for B, H, W in WORKLOADS:
        for net, small in (("full", False), ("small", True)):
            for prec in PRECS:
                tag = f"{net}/{B}x{H}x{W}/{prec}"
                # the feature encoder (InstanceNorm: both features wherever the conv takes them) on both frames,
                # the context encoder (its norm folded: a RELU epilogue) on one
                for name, cin, n, k, stride, ds in _encoder(small):
                    h, w = _down(H, ds), _down(W, ds)
                    out.append(_case(f"{tag}/fnet.{name}", 2 * B, h, w, cin, n, (k, k), stride, prec,
                                     stats=True, in_norm=True))
                    out.append(_case(f"{tag}/cnet.{name}", B, h, w, cin, n, (k, k), stride, prec,
                                     epilogue=_lib.EPI_RELU))
                for name, cin, n, k in _update(small):
                    out.append(_case(f"{tag}/upd.{name}", B, _down(H, 8), _down(W, 8), cin, n, k, 1, prec))
    return out


def _random_cases():
    """Groups of four convs on one B, H, W (so that each has a pair partner); every second one copies its
    neighbour's kernel, stride and precision half the time (only such convs share a launch)."""
    rng = random.Random(SEED)
    out = []
    for g in range(N_RANDOM // 4):
        B, H, W = rng.randint(1, 8), rng.randint(1, 300), rng.randint(1, 300)
        prev = None
        for j in range(4):
            k, stride, prec = rng.choice(RANDOM_K), rng.choice((1, 1, 1, 2)), rng.choice(PRECS)
            if prev is not None and j % 2 == 1 and rng.random() < 0.5:
                k, stride, prec = prev
            prev = (k, stride, prec)
            out.append(_case(f"random/{g}.{j}", B, H, W, 4 * rng.randint(1, 96), rng.choice(RANDOM_N), k, stride, prec,
                             epilogue=rng.choice((_lib.EPI_LINEAR, _lib.EPI_RELU)), scaled=rng.random() < 0.75,
                             stats=rng.random() < 0.5, in_norm=rng.random() < 0.5))
    return out


def cases():
    return _table_cases() + _workload_cases() + _random_cases()


def bare_params(c, slot=0):
    """conv_forms.host_params of the conv without features; slot moves the stand-in operands (1 TiB apart: the
    operands of two slots never meet)."""
    p = CF.host_params(CF.Conv(c.name, c.B, c.H, c.W, c.cin, c.n, c.kh, c.kw, c.stride, c.prec, None), c.epilogue)
    base = (1 + 4 * slot) << 40
    p.in0, p.weight, p.out = base, base + (1 << 40), base + (2 << 40)
    if p.weight_s is not None:
        p.weight_s = (base + (3 << 40)) if c.scaled else None
    return p


def _fmt(f):
    return ",".join(str(v) for v in f.astuple())


def line_of(lib, c, partner):
    bare, p = bare_params(c), bare_params(c)
    if c.in_norm and lib.raft_conv2d_in_norm_ok(ctypes.byref(bare)):
        p.in_norm, p.in_norm_relu = 5 << 40, 1
    unset = bare_params(c)
    unset.in_norm, unset.in_norm_relu = p.in_norm, p.in_norm_relu
    slots = lib.raft_conv2d_stats_slots(ctypes.byref(unset))   # stats_part unset, in_norm as the launch has it
    if c.stats and slots > 0:
        p.stats_part, p.stats_ld = 6 << 40, c.n + 4
    f = _lib.ConvForm()
    rc = lib.raft_conv2d_form(ctypes.byref(p), ctypes.byref(f))
    text = (f"{c.name} rc={rc} form={_fmt(f)} slots={slots} rows={lib.raft_conv2d_halo_tile_rows(ctypes.byref(p))} "
            f"m={lib.raft_conv2d_halo_tiles_per_wg(ctypes.byref(p))} norm={lib.raft_conv2d_in_norm_ok(ctypes.byref(p))}")
    if partner is not None:
        ff = (_lib.ConvForm * 2)()
        one = ctypes.c_int(-1)
        prc = lib.raft_conv2d_pair_form(ctypes.byref(bare), ctypes.byref(bare_params(partner, slot=4)), ff,
                                        ctypes.byref(one))
        text += f" | pair({partner.name}) rc={prc} one={one.value} f0={_fmt(ff[0])} f1={_fmt(ff[1])}"
    return text, rc


def text_of_this_process():
    """The signature text under this process's environment, and its random cases' accepted count."""
    lib = _lib.load()
    cs = cases()
    lines, ok_random = [], 0
    for i, c in enumerate(cs):
        nxt = cs[i + 1] if i + 1 < len(cs) else None
        partner = nxt if nxt is not None and (nxt.B, nxt.H, nxt.W) == (c.B, c.H, c.W) else None
        text, rc = line_of(lib, c, partner)
        lines.append(text)
        ok_random += c.name.startswith("random/") and rc == 0
    return "\n".join(lines) + "\n", ok_random


def text_of(setting):
    """The signature text of one setting, computed in a fresh child process."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    if setting != "default":
        k, v = setting.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE,
                       timeout=CHILD_TIMEOUT, check=True)
    return r.stdout.decode()


def digest(text):
    return {"sha256": hashlib.sha256(text.encode()).hexdigest(), "lines": text.count("\n")}


def compute():
    return {s: digest(text_of(s)) for s in SETTINGS}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", metavar="FILE", help="record every setting's signature into FILE")
    g.add_argument("--check", metavar="FILE", help="compare against FILE; exit 1 where a setting differs")
    g.add_argument("--dump", metavar="SETTING", help="print one setting's text, one case per line")
    g.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        sys.stdout.write(text_of_this_process()[0])
        return 0
    if a.dump:
        if a.dump not in SETTINGS:
            ap.error(f"unknown setting {a.dump!r}; known:\n  " + "\n  ".join(SETTINGS))
        sys.stdout.write(text_of(a.dump))
        return 0
    got = compute()
    if a.write:
        with open(a.write, "w") as fh:
            json.dump(got, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print(f"{a.write}: {len(got)} settings, {got['default']['lines']} cases each")
        return 0
    with open(a.check) as fh:
        recorded = json.load(fh)
    bad = [s for s in SETTINGS if recorded.get(s) != got[s]]
    for s in bad:
        print(f"DIFFERS: {s}")
    print(f"{len(SETTINGS)} settings, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
