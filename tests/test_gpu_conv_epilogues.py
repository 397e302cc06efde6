"""Every conv epilogue on every kernel form, at kernel level.

All conv arithmetic leaves the kernels through one of seven epilogues (conv_common.hpp), each optionally with the
add0 addend; the code is instantiated per kernel form (halo tiles of 32 / 64 / 128 columns, 8 or 16 rows, one or
several per work-group, 4 or 8 loaders, the K-split form, the GEMM kernel with one or two K-groups, the small-N
VALU kernels, the stem), each with its own row / column ownership and masking.  For every form of conv_forms.TABLE
(asserted through raft_conv2d_form before each launch) and every epilogue the kernel accepts, with operands laid
out as the engine lays them out (column sub-views of wider buffers with other leading dimensions, GRU_Q in place
over two input segments, GRU_ZR's aux0 inside its own input rows, ADD_TO_OUT on a pre-filled destination):

(a) against fp64: the conv in fp64 by torch (once per shape), the epilogue applied in fp64.  Bound: CONV_TOL[prec] x
    max(1, max|v_ref|) x max(1, |alpha|), v_ref the pre-activation value -- every epilogue is 1-Lipschitz in v
    given |h| <= 1 and z in [0, 1] (h is drawn through tanh, z through sigmoid), so the conv tolerance carries over;
(b) the epilogue alone: the same conv run with EPI_LINEAR, alpha 1, no add0 gives the kernel's own v bit for bit
    (same form, deterministic).  The exact epilogues (LINEAR x alpha, RELU, RESID_RELU, ADD_TO_OUT, the relu half of
    TANH_RELU), evaluated in fp32 in the kernel's order on that v, must agree bit for bit (2^-22 relative, one fp32
    rounding either side, would cover another fma contraction; all cases measure bit-equal); the sigmoid / tanh ones, evaluated in fp64, within 1e-5 absolute (the bound of
    test_conv2d_two_segments_and_gru_epilogues for the fast activations).  (b) keeps bf16 sharp, where (a) allows 3e-2.

Unwritten columns and guard rows of every written buffer hold a sentinel and must stay untouched.  The range-flag
tests raise / do not raise the f16x3 guard on each kernel that has it.  Measured errors: DESIGN.md."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_forms as CF
from test_gpu_parity import CONV_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0     # sentinel of unwritten columns / guard rows
G = 4           # guard rows above and below every buffer
EXACT_REL = 2.0 ** -22
FAST_ABS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    lib = _lib.load()
    # the table is written for the default forms (K-split on, 8 loaders)
    assert (lib.raft_conv2d_set_halo_ks(0), lib.raft_conv2d_set_halo_loaders(0)) == (2, 8)
    yield
    for cached in (_conv_data, _packed, _kernel_v):   # the shared references: not kept for the modules after this one
        cached.cache_clear()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- data (shared, never modified)


def _key(c):
    return (c.B, c.H, c.W, c.cin, c.n, c.kh, c.kw, c.stride)


@functools.lru_cache(maxsize=None)
def _conv_data(key):
    """Per conv shape: input, weight, bias, the fp64 conv (+ bias) as rows [npix, n] and the random epilogue
    operands, all on the device.  Shared by every precision and epilogue of the shape."""
    B, H, W, cin, n, kh, kw, stride = key
    seed = sum((i + 1) * 7919 * v for i, v in enumerate(key)) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(B, cin, H, W, generator=g))
    w = torch.randn(n, cin, kh, kw, generator=g) / np.sqrt(cin * kh * kw)
    b = torch.randn(n, generator=g)
    pad = ((kh - 1) // 2, (kw - 1) // 2)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride, pad)
    ho, wo = ref.shape[-2:]
    npix = B * ho * wo
    gd = torch.Generator(device=DEV).manual_seed(seed + 1)

    def rnd():
        return torch.randn(npix, n, generator=gd, device=DEV)

    return dict(
        x=x, w=w, b=b, pad=pad, ho=ho, wo=wo, npix=npix, npix_in=B * H * W,
        xrows=x.permute(0, 2, 3, 1).reshape(B * H * W, cin).contiguous().to(DEV),
        v64=ref.permute(0, 2, 3, 1).reshape(npix, n).contiguous().to(DEV),
        add0=rnd(), res=rnd(), h=torch.tanh(rnd()), z=torch.sigmoid(rnd()), prev=rnd())


@functools.lru_cache(maxsize=None)
def _packed(key, prec):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    d = _conv_data(key)
    pc = K.pack_conv(d["w"], d["b"], key[7], d["pad"], device=DEV)
    pc.precision = _lib.PRECISIONS[prec]
    return pc


def _buf(rows, ld, fill=SENT):
    """A [rows, ld] view with G guard rows above and below, everything = fill; returns (whole, view)."""
    whole = torch.full((rows + 2 * G, ld), fill, device=DEV)
    return whole, whole[G:G + rows]


def _up4(v):
    return -(-v // 4) * 4


# ----------------------------------------------------------------------------- the epilogues, restated


VARIANTS = {  # name: (epilogue, add0)
    "linear": ("LINEAR", False), "linear_add0": ("LINEAR", True),
    "relu": ("RELU", False), "relu_add0": ("RELU", True),
    "resid": ("RESID_RELU", False), "resid_add0": ("RESID_RELU", True),
    "zr": ("GRU_ZR", False), "zr_add0": ("GRU_ZR", True),
    "q": ("GRU_Q", False), "q_add0": ("GRU_Q", True),
    "tanh_relu": ("TANH_RELU", False), "tanh_relu_add0": ("TANH_RELU", True),
    "add_to_out": ("ADD_TO_OUT", False), "add_to_out_add0": ("ADD_TO_OUT", True),
}
SPLIT_EPIS = ("GRU_ZR", "TANH_RELU")
FAST_EPIS = ("GRU_ZR", "GRU_Q", "TANH_RELU")


def _variants_of(c):
    if c.form[0] == CF.STEM:
        return ["linear", "relu"]            # all the stem accepts (LINEAR at alpha 1)
    if c.n <= 4:
        return [v for v, (e, _) in VARIANTS.items() if e not in SPLIT_EPIS]   # split % 32 == 0 needs n > 32
    return list(VARIANTS)


def _split_of(c, epi, add0):
    """With add0 (as the engine runs them): the halves of the product (128 | 128 at N = 256) or 64 | rest where
    the half is no multiple of 32 (N = 100: 64 | 36, N = 126: 64 | 62); without: 32 | rest."""
    if epi not in SPLIT_EPIS:
        return 0
    if not add0:
        return 32
    return c.n // 2 if (c.n // 2) % 32 == 0 else 64


def _apply(epi, t, alpha, split, res, h, z, prev):
    """The epilogue on the pre-activation t (= conv + bias + add0) in t's dtype, in the kernel's order of
    operations (conv_common.hpp tile_epilogue); returns (out columns, out1 columns or None)."""
    if epi == "LINEAR":
        return alpha * t, None
    if epi == "RELU":
        return torch.relu(t), None
    if epi == "RESID_RELU":
        return torch.relu(res + torch.relu(t)), None
    if epi == "GRU_ZR":
        return torch.sigmoid(t[:, :split]), torch.sigmoid(t[:, split:]) * h
    if epi == "GRU_Q":
        return (1.0 - z) * h + z * torch.tanh(t), None
    if epi == "TANH_RELU":
        return torch.tanh(t[:, :split]), torch.relu(t[:, split:])
    if epi == "ADD_TO_OUT":
        return prev + t, None
    raise ValueError(epi)


# ----------------------------------------------------------------------------- one launch


def _inputs(c, d, two_seg, aux_cols, gen):
    """The conv's input rows as the engine holds them.  One segment: X[:, :cin] of a wider buffer whose further
    columns (tanh-drawn) serve GRU_ZR's aux0 = X[:, :aux_cols].  Two segments (GRU_Q): seg 0 a buffer of its own
    (r * h), seg 1 the columns after h of the [h | x] buffer whose h columns are the in-place output."""
    from raft_optical_flow_amd import kernels as K
    cin, n, rows = c.cin, c.n, d["npix_in"]
    if not two_seg:
        ld = cin if cin % 4 else _up4(max(cin, aux_cols)) + 8   # (the stem reads packed 3-channel rows)
        whole, X = _buf(rows, ld)
        if ld > cin:
            X[:, cin:] = torch.tanh(torch.randn(rows, ld - cin, generator=gen, device=DEV))
        X[:, :cin] = d["xrows"]
        return dict(src0=K.Rows(X, 0, cin), src1=None, X=X)
    c0 = 32 * max(1, cin // 64)  # seg 0 % 32 == 0 (VEC): 32 | 32, 32 | 64, 128 | 128
    c1 = cin - c0
    _, RH = _buf(rows, c0 + 4)
    RH[:, :c0] = d["xrows"][:, :c0]
    n4 = _up4(n)
    whole, HX = _buf(rows, n4 + c1 + 4)
    HX[:, n4:n4 + c1] = d["xrows"][:, c0:]
    return dict(src0=K.Rows(RH, 0, c0), src1=K.Rows(HX, n4, c1), HX=HX, HX_whole=whole)


def _launch(c, p):
    """Asserts the form raft_conv2d_form reports for these very params, then launches them."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    form = _lib.conv_form(p).astuple()
    assert form == c.form, (c.name, form, c.form)
    K.conv_launch(p)(K.stream_handle())


@functools.lru_cache(maxsize=None)
def _kernel_v(name, two_seg):
    """The kernel's own v = conv + bias of the case (EPI_LINEAR, alpha 1, no add0; same form and segments)."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    c = CF.BY_NAME[name]
    d = _conv_data(_key(c))
    gen = torch.Generator(device=DEV).manual_seed(1)
    src = _inputs(c, d, two_seg, 0, gen)
    out = torch.full((d["npix"], c.n), SENT, device=DEV)
    p = K.conv_params(_packed(_key(c), c.prec), src["src0"], c.B, c.H, c.W, K.Rows(out), src1=src["src1"],
                      epilogue=_lib.EPI_LINEAR, alpha=1.0)
    _launch(c, p)
    torch.cuda.synchronize()
    return out


def _unchanged_outside(whole, before, col0, ncols):
    """Everything of `whole` outside view rows x columns [col0, col0 + ncols) still equals `before`."""
    a, b = whole.clone(), before.clone()
    a[G:-G, col0:col0 + ncols] = 0
    b[G:-G, col0:col0 + ncols] = 0
    return torch.equal(a, b)


def _run_variant(c, variant):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    epi, with_add0 = VARIANTS[variant]
    d = _conv_data(_key(c))
    n, npix = c.n, d["npix"]
    assert npix <= d["npix_in"]
    alpha = 1.0 if c.form[0] == CF.STEM else 0.25   # 0.25: the mask head's value
    split = _split_of(c, epi, with_add0)
    two_seg = epi == "GRU_Q"
    gen = torch.Generator(device=DEV).manual_seed(2)
    src = _inputs(c, d, two_seg, n - split if epi == "GRU_ZR" else 0, gen)
    kw = dict(src1=src["src1"], epilogue=getattr(_lib, "EPI_" + epi), alpha=alpha, split=split)
    written = []  # (whole buffer, its state before the launch, first written column, written columns, expected key)

    # the destination(s): column sub-views, first columns 4 (out) and 3 (out1), other leading dimensions
    if two_seg:
        whole, HX = src["HX_whole"], src["HX"]
        HX[:npix, :n] = d["h"]                       # in place: out aliases aux0 (h), as engine.py runs the GRU
        out = K.Rows(HX, 0, n)
        kw.update(aux0=out)
        h = d["h"]
        written.append((whole, 0, n, "out"))
    else:
        whole, O = _buf(npix, n + 12)
        ncol = split if split else n
        if epi == "ADD_TO_OUT":
            O[:, 4:4 + n] = d["prev"]
        out = K.Rows(O, 4, ncol)
        written.append((whole, 4, ncol, "out"))
    if split:
        whole1, O1 = _buf(npix, n - split + 7)
        kw.update(out1=K.Rows(O1, 3, n - split))
        written.append((whole1, 3, n - split, "out1"))
    # the read-only operands
    if with_add0:
        _, A = _buf(npix, n + 5)
        A[:, 1:1 + n] = d["add0"]
        kw.update(add0=K.Rows(A, 1, n))
    if epi == "RESID_RELU":
        _, R = _buf(npix, n + 11)
        R[:, 8:8 + n] = d["res"]
        kw.update(aux0=K.Rows(R, 8, n))
    if epi == "GRU_ZR":
        kw.update(aux0=K.Rows(src["X"], 0, n - split))   # a sub-view of the conv's own input rows
        h = src["X"][:npix, :n - split].clone()
        assert float(h.abs().max()) <= 1.0
    if epi == "GRU_Q":
        _, Z = _buf(npix, n + 6)
        Z[:, 5:5 + n] = d["z"]
        kw.update(aux1=K.Rows(Z, 5, n))
    if epi not in ("GRU_ZR", "GRU_Q"):
        h = None
    before = [w_.clone() for w_, *_ in written]

    p = K.conv_params(_packed(_key(c), c.prec), src["src0"], c.B, c.H, c.W, out, **kw)
    _launch(c, p)
    torch.cuda.synchronize()

    got = {"out": out.t[:npix, out.off:out.off + out.c]}
    if split:
        got["out1"] = O1[:, 3:3 + n - split]
    for (w_, col0, ncols, _), b_ in zip(written, before):
        assert _unchanged_outside(w_, b_, col0, ncols), (c.name, variant, "wrote outside its rows / columns")
    if two_seg:  # the sentinel columns of the [h | x] buffer in particular
        n4 = _up4(n)
        assert bool((src["HX"][:, n:n4] == SENT).all()) and bool((src["HX"][:, n4 + c.cin - src["src0"].c:] == SENT).all())

    # (a) against fp64
    add64 = d["add0"].double() if with_add0 else 0.0
    t64 = d["v64"] + add64
    ops64 = dict(res=d["res"].double(), h=None if h is None else h.double(), z=d["z"].double(),
                 prev=d["prev"].double())
    ref = dict(zip(("out", "out1"), _apply(epi, t64, alpha, split, **ops64)))
    bound_a = CONV_TOL[c.prec] * max(1.0, float(t64.abs().max())) * max(1.0, abs(alpha))
    err_a = max(float((got[k].double() - ref[k]).abs().max()) for k in got)

    # (b) the epilogue alone, on the kernel's own v
    v = _kernel_v(c.name, two_seg)
    t32 = v + d["add0"] if with_add0 else v
    err_exact = err_fast = 0.0
    bit_equal = True
    if epi in FAST_EPIS:
        t = t32.double()
        exp = dict(zip(("out", "out1"), _apply(epi, t, alpha, split, **ops64)))
        for k in got:
            if epi == "TANH_RELU" and k == "out1":   # the relu half is exact
                e32 = torch.relu(t32[:, split:])
                bit_equal &= torch.equal(got[k], e32)
                err_exact = max(err_exact, float(((got[k] - e32).abs() / e32.abs().clamp_min(1e-30)).max()))
            else:
                err_fast = max(err_fast, float((got[k].double() - exp[k]).abs().max()))
    else:
        e32 = _apply(epi, t32, alpha, split, res=d["res"], h=None, z=None, prev=d["prev"])[0]
        bit_equal = torch.equal(got["out"], e32)
        err_exact = float(((got["out"] - e32).abs() / e32.abs().clamp_min(1e-30)).max())
    print(f"EPIERR case={c.name} prec={c.prec} epi={epi} add0={int(with_add0)} a={err_a:.3e} bound_a={bound_a:.3e} "
          f"b_exact_rel={err_exact:.3e} bit_equal={int(bit_equal)} b_fast_abs={err_fast:.3e}")
    assert err_a < bound_a, (c.name, variant, err_a, bound_a)
    # the issue's bound for the exact epilogues is 2^-22 relative (room for another fma contraction between the
    # two runs); every case measured bit-equal on MI355X, so equality is what is asserted
    assert bit_equal and err_exact <= EXACT_REL, (c.name, variant, err_exact)
    assert err_fast < FAST_ABS, (c.name, variant, err_fast)


MATRIX = [(c.name, v) for c in CF.TABLE for v in _variants_of(c)]


@pytest.mark.parametrize("name,variant", MATRIX, ids=[f"{n}-{v}" for n, v in MATRIX])
def test_epilogue_on_form(name, variant):
    _run_variant(CF.BY_NAME[name], variant)


# ----------------------------------------------------------------------------- the f16x3 range flag


FLAG_CASES = ["h32-3x3-f16x3", "h64-3x3-f16x3", "big-3x3-f16x3", "gemm2-3x3s2-f16x3", "stem-f16x3"]


def _flag_run(c, w, b, x):
    """LINEAR (alpha 1) conv of x with (w, b) in the case's form; returns (range flag, output rows)."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, cin, H, W = x.shape
    pad = CF.pad_of(c)
    pc = K.pack_conv(w, b, c.stride, pad, device=DEV)
    pc.precision = _lib.PREC_F16X3
    src = K.Rows(x.permute(0, 2, 3, 1).reshape(B * H * W, cin).contiguous().to(DEV))
    ho, wo = (H + 2 * pad[0] - c.kh) // c.stride + 1, (W + 2 * pad[1] - c.kw) // c.stride + 1
    out = K.Rows(torch.full((B * ho * wo, c.n), SENT, device=DEV))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = K.conv_params(pc, src, B, H, W, out, epilogue=_lib.EPI_LINEAR, alpha=1.0, range_flag=flag)
    assert p.range_flag
    form = _lib.conv_form(p).astuple()
    assert form == c.form, (c.name, form)
    K.conv_launch(p)(K.stream_handle())
    torch.cuda.synchronize()
    return int(flag.item()), out.t


@pytest.mark.parametrize("name", FLAG_CASES)
def test_range_flag_raised_only_by_in_image_outputs_above_the_limit(name):
    """One channel above 2^15 raises the flag; the same channel just below leaves it 0; a NaN output leaves it 0
    (raft_hip.h: NaN does not raise it)."""
    from raft_optical_flow_amd import _lib
    c = CF.BY_NAME[name]
    d = _conv_data(_key(c))
    ch = c.n - 3
    cmax = float((d["v64"][:, ch] - float(d["b"][ch])).abs().max())   # the channel's conv without its bias
    assert cmax < 100.0
    for bias, want in ((4.0e4, 1), (_lib.RANGE_LIMIT - cmax - 1.0, 0), (float("nan"), 0)):
        b = d["b"].clone()
        b[ch] = bias
        flag, out = _flag_run(c, d["w"], b, d["x"])
        col = out[:, ch]
        if want:
            assert float(col.abs().min()) > _lib.RANGE_LIMIT
        elif bias == bias:
            # just below: every output of the channel is within 2 cmax + 2 of the limit and none is above it
            assert _lib.RANGE_LIMIT - 2.0 * cmax - 2.0 < float(col.min()) and float(col.max()) < _lib.RANGE_LIMIT
        else:
            assert bool(torch.isnan(col).all())
        assert flag == want, (name, bias, flag)


@pytest.mark.parametrize("name", FLAG_CASES)
def test_range_flag_ignores_masked_rows(name):
    """Rows of a tile past the image's edge cannot raise the flag: the input is large only from the first image
    row that, under the top tap row, feeds no in-image output but feeds the output row just past the edge
    (stride 1: the last image row), and the weights are non-zero only on the top tap row.  Checked in fp64:
    every in-image output is far below the limit while the row past the edge would be far above it."""
    from raft_optical_flow_amd import _lib
    c = CF.BY_NAME[name]
    B, cin = c.B, c.cin
    H = c.H + 1 if name.startswith("gemm2") else c.H     # (stride 2, pad 1: an even height has such a row)
    W = c.W
    pad = CF.pad_of(c)
    ho = (H + 2 * pad[0] - c.kh) // c.stride + 1
    r_big = c.stride * ho - pad[0]   # the input row under tap row 0 of output row ho, the first past the edge
    assert 0 < r_big <= H - 1
    g = torch.Generator().manual_seed(11)
    x = torch.tanh(torch.randn(B, cin, H, W, generator=g))
    x[:, :, r_big:] = 4.0e4 * (1.0 + 0.5 * torch.rand(B, cin, H - r_big, W, generator=g))   # (below f16's 65504)
    w = torch.zeros(c.n, cin, c.kh, c.kw)
    w[:, :, 0] = torch.rand(c.n, cin, c.kw, generator=g) + 0.5
    b = torch.zeros(c.n)
    ref = F.conv2d(x.double(), w.double(), b.double(), c.stride, pad)
    assert float(ref.abs().max()) < 0.1 * _lib.RANGE_LIMIT
    past = F.conv2d(F.pad(x.double(), (0, 0, 0, c.stride)), w.double(), b.double(), c.stride, pad)
    assert past.shape[2] > ho and float(past[:, :, ho].abs().min()) > 2.0 * _lib.RANGE_LIMIT
    flag, out = _flag_run(c, w, b, x)
    got = out.view(B, ho, -1, c.n).permute(0, 3, 1, 2).double().cpu()
    assert float((got - ref).abs().max()) < CONV_TOL["f16x3"] * max(1.0, float(ref.abs().max()))
    assert flag == 0, name
