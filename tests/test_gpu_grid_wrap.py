"""The grid-stride wrap of the elementwise kernels: every launch here has just over 65,536 blocks x 256 threads
= 16,777,216 work items (and not a multiple of 256), so the grid is capped, every thread loops a second time
and the tail is ragged.  Production reaches this at 1080p with B >= 2 (raft_prep_images, raft_nchw_to_nhwc,
raft_instnorm_apply's vector form, which also indexes in 32 bits there).

Each case only has to show that every element is written once and correctly: the reference is the same formula
in plain torch ops on the device (fp64 where the formula rounds), under the tolerances of the small-shape tests
(test_gpu_norm_apply / test_gpu_upsample / test_gpu_layout / test_gpu_caller); copies and layout changes must be
equal.  Outputs are pre-filled with -7.0 and a tail behind them must keep it.  Each case stays far below 4 GB
of device memory and frees it before the next."""
import gc

import pytest
import torch
import torch.nn.functional as F

import elementwise_oracle as EO

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0
TAIL = 256
CAP = 65536 * 256


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


@pytest.fixture(autouse=True)
def _free():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def call(name, *args):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    _lib.call(name, *args, K.stream_handle())
    torch.cuda.synchronize()


def wraps(items):
    """The case is what it claims: a second trip through the grid-stride loop with a ragged tail."""
    assert CAP < items < CAP + CAP // 64 and items % 256 != 0, items
    return items


def sentinel(n):
    return torch.full((n + TAIL,), SENT, device=DEV)


def take(buf, n):
    assert bool((buf[n:] == SENT).all()), "wrote past the output"
    return buf[:n]


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def measured(ref32, ref64, floor):
    e_ref = maxerr(ref32, ref64)
    return max(4 * e_ref, floor), e_ref


def test_prep_images_16779606():
    B, H, W = 1, 1399, 1999
    n = wraps(2 * B * H * W * 3)
    a, b = rand(B, 3, H, W, seed=1).mul(60).add(128).clamp(0, 255), rand(B, 3, H, W, seed=2).mul(60).add(128).clamp(0, 255)
    out = sentinel(n)
    call("raft_prep_images", a.data_ptr(), b.data_ptr(), out.data_ptr(), B, H, W)
    ref = (2.0 * (torch.cat([a, b]).double() / 255.0) - 1.0).permute(0, 2, 3, 1).reshape(-1)
    assert maxerr(take(out, n), ref) <= 3 * EO.U


def test_init_coords_and_flow_from_coords_16781310():
    B, H, W = 1, 2049, 4095
    n = wraps(B * H * W * 2)
    flow = rand(B, 2, H, W, seed=3, scale=7.0)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32),
                            torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None]
    coords = sentinel(n)
    call("raft_init_coords", coords.data_ptr(), flow.data_ptr(), B, H, W)
    want = grid + flow                                          # one fp32 add per element
    assert torch.equal(take(coords, n).view(B, H, W, 2), want.permute(0, 2, 3, 1))
    back = sentinel(n)
    call("raft_flow_from_coords", coords.data_ptr(), back.data_ptr(), B, H, W)
    assert torch.equal(take(back, n).view(B, 2, H, W), want - grid)
    plain = sentinel(n)
    call("raft_init_coords", plain.data_ptr(), None, B, H, W)
    assert torch.equal(take(plain, n).view(B, H, W, 2), grid.permute(0, 2, 3, 1))


def test_convex_upsample_16842816():
    """The mask is 263,169 rows x 576 floats = 0.6 GB; the fp64 reference goes a chunk of pixels at a time.
    Bound as in test_gpu_upsample: max(4 * E_ref, 16 * 2^-24 * max|ref|), E_ref from the same torch formula in
    float32.  Seen on an MI355X: E_ref 1.3e-4, bound 5.4e-4, kernel 1.2e-4."""
    B, H, W = 1, 513, 513
    n = wraps(B * 64 * H * W)
    flow = rand(B, 2, H, W, seed=4, scale=10.0)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32),
                            torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None]
    coords = (grid + flow).permute(0, 2, 3, 1).contiguous()
    f32 = coords.permute(0, 3, 1, 2) - grid                     # what the kernel sees
    mask = rand(B * H * W, 576, seed=5, scale=10.0)
    out = sentinel(2 * n)
    call("raft_convex_upsample", coords.data_ptr(), mask.data_ptr(), 576, out.data_ptr(), B, H, W)
    got = take(out, 2 * n).view(B, 2, 8 * H, 8 * W)
    ref = EO.upsample_flow_torch(f32, mask, torch.float64)
    bound, e_ref = measured(EO.upsample_flow_torch(f32, mask, torch.float32), ref, 16 * EO.U * float(ref.abs().max()))
    err = maxerr(got, ref)
    print(f"convex wrap: E_ref {e_ref:.3e} bound {bound:.3e} gpu err {err:.3e}")
    assert err <= bound


def test_upflow8_16866432():
    """Both bounds of test_gpu_upsample.test_upflow8.  Seen on an MI355X: 0 against the float32 formula (bound
    1.7e-4); E_ref 9.5e-3 and as much against fp64 (bound 3.8e-2)."""
    B, H, W = 1, 363, 363
    n = wraps(B * 128 * H * W)
    flow = rand(B, 2, H, W, seed=6, scale=10.0)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32),
                            torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None]
    coords = (grid + flow).permute(0, 2, 3, 1).contiguous()
    f32 = coords.permute(0, 3, 1, 2) - grid
    out = sentinel(n)
    call("raft_upflow8", coords.data_ptr(), out.data_ptr(), B, H, W)
    got = take(out, n).view(B, 2, 8 * H, 8 * W)
    ref32, ref64 = EO.upflow8_torch(f32, torch.float32), EO.upflow8_torch(f32, torch.float64)
    big = float(ref64.abs().max())
    bound, e_ref = measured(ref32, ref64, 16 * EO.U * big)
    e32, e64 = maxerr(got, ref32), maxerr(got, ref64)
    print(f"upflow8 wrap: vs fp32 {e32:.3e} (bound {8 * EO.U * big:.3e}); E_ref {e_ref:.3e}, vs fp64 {e64:.3e} "
          f"(bound {bound:.3e})")
    assert e32 <= 8 * EO.U * big
    assert e64 <= bound


def test_nchw_nhwc_16784105():
    B, C, H, W, ld = 1, 5, 1733, 1937, 8
    n = wraps(B * C * H * W)
    x = rand(B, C, H, W, seed=7)
    rows = sentinel(B * H * W * ld)
    call("raft_nchw_to_nhwc", x.data_ptr(), rows.data_ptr(), ld, B, C, H, W)
    r = take(rows, B * H * W * ld).view(B * H * W, ld)
    assert torch.equal(r[:, :C], x.permute(0, 2, 3, 1).reshape(-1, C))
    assert bool((r[:, C:] == SENT).all())
    back = sentinel(n)
    call("raft_nhwc_to_nchw", rows.data_ptr(), ld, back.data_ptr(), B, C, H, W)
    assert torch.equal(take(back, n).view(B, C, H, W), x)


def test_avgpool2_nhwc_16784105():
    B, C, Ho, Wo = 1, 5, 1733, 1937
    H, W = 2 * Ho + 1, 2 * Wo + 1                               # odd sizes floor
    n = wraps(B * Ho * Wo * C)
    x = rand(B, H, W, C, seed=8, scale=3.0)
    out = sentinel(n)
    call("raft_avgpool2_nhwc", x.data_ptr(), out.data_ptr(), B, H, W, C)
    v = x[:, :2 * Ho, :2 * Wo]
    want = (((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + v[:, 1::2, 0::2]) + v[:, 1::2, 1::2]) * 0.25   # / 4 is exact
    assert torch.equal(take(out, n).view(B, Ho, Wo, C), want)


def apply_reference(x, st, res, rst, gamma=None, beta=None, rows=1 << 20):
    """relu(norm(res) + relu(norm(x))) (relu_mode 2, resid_stats given; rst None: the raw residual) in fp64, with
    the per-element path magnitude, for x / res [B, HW, C] and stats [B, C, 2]; yields (row slice, ref, mag)
    per chunk of pixels to bound the memory."""
    B, HW, C = x.shape
    for b in range(B):
        for s in range(0, HW, rows):
            sl = (b, slice(s, min(s + rows, HW)))
            d = x[sl].double() - st[b, :, 0].double()
            v = d * st[b, :, 1].double()
            mag = torch.maximum(d.abs(), v.abs())
            if gamma is not None:
                v = v * gamma.double()
                mag = torch.maximum(mag, v.abs())
                v = v + beta.double()
                mag = torch.maximum(mag, v.abs())
            v = v.clamp(min=0)
            r = res[sl].double()
            mag = torch.maximum(mag, r.abs())
            if rst is not None:
                r = r - rst[b, :, 0].double()
                mag = torch.maximum(mag, r.abs())
                r = r * rst[b, :, 1].double()
                mag = torch.maximum(mag, r.abs())
            v = r + v
            mag = torch.maximum(mag, v.abs())
            yield sl, v.clamp(min=0), mag


def apply_case(B, HW, C, seed):
    x = rand(B, HW, C, seed=seed, scale=2.0) + torch.linspace(-90, 90, C, device=DEV)
    res = rand(B, HW, C, seed=seed + 1, scale=3.0) - torch.linspace(-50, 50, C, device=DEV)
    st = torch.stack([torch.linspace(-90, 90, C, device=DEV).expand(B, C) + rand(B, C, seed=seed + 2) * 0.5,
                      rand(B, C, seed=seed + 3).abs() * 0.3 + 0.4], -1).contiguous()
    rst = torch.stack([-torch.linspace(-50, 50, C, device=DEV).expand(B, C) + rand(B, C, seed=seed + 4) * 0.5,
                       rand(B, C, seed=seed + 5).abs() * 0.2 + 0.3], -1).contiguous()
    return x, st, res, rst


@pytest.mark.parametrize("form,B,HW,C,items", [
    ("scalar", 2, 1398103, 6, 2 * 1398103 * 6),          # C = 6: the scalar kernel, B*HW*C items
    ("vector", 2, 4194321, 8, 2 * 4194321 * 8 // 4),     # aligned, C % 4 == 0: the vector kernel, B*HW*C/4 items
], ids=lambda v: str(v))
def test_instnorm_apply(form, B, HW, C, items):
    """Both kernels past the cap (the vector case is 67 M floats in and out, 32-bit indexed): relu_mode 2; the
    scalar case with a normalised residual, the vector case with a raw one.  Bound as in test_gpu_norm_apply:
    5 * 2^-24 * mag * 2 per element."""
    wraps(items)
    x, st, res, rst = apply_case(B, HW, C, seed=20)
    if form == "vector":
        rst = None
    out = sentinel(B * HW * C)
    call("raft_instnorm_apply", x.data_ptr(), C, st.data_ptr(), res.data_ptr(), C, None if rst is None else rst.data_ptr(),
         2, out.data_ptr(), C, B, HW, C)
    got = take(out, B * HW * C).view(B, HW, C)
    for sl, ref, mag in apply_reference(x, st, res, rst):
        assert bool(((got[sl].double() - ref).abs() <= 5 * EO.U * mag * 2).all()), sl


def test_norm_apply_affine_16777236():
    """9 * 2^-24 * mag * 2 per element, as in test_gpu_norm_apply."""
    B, HW, C = 2, 1398103, 6
    wraps(B * HW * C)
    x, st, res, rst = apply_case(B, HW, C, seed=30)
    gamma, beta = rand(C, seed=40) * 1.5, rand(C, seed=41) * 2.0
    out = sentinel(B * HW * C)
    call("raft_norm_apply_affine", x.data_ptr(), C, st.data_ptr(), gamma.data_ptr(), beta.data_ptr(), res.data_ptr(), C,
         rst.data_ptr(), None, None, 2, out.data_ptr(), C, B, HW, C)
    got = take(out, B * HW * C).view(B, HW, C)
    for sl, ref, mag in apply_reference(x, st, res, rst, gamma, beta):
        assert bool(((got[sl].double() - ref).abs() <= 9 * EO.U * mag * 2).all()), sl


def test_pad_replicate_16822197():
    NC, H, W, top, bottom, left, right = 3, 2360, 2366, 1, 2, 3, 4
    Ho, Wo = H + top + bottom, W + left + right
    n = wraps(NC * Ho * Wo)
    x = rand(1, NC, H, W, seed=9)
    out = sentinel(n)
    call("raft_pad_replicate", x.data_ptr(), out.data_ptr(), NC, H, W, top, bottom, left, right)
    assert torch.equal(take(out, n).view(1, NC, Ho, Wo), F.pad(x, (left, right, top, bottom), mode="replicate"))


def test_bilinear_sample_16785409():
    """C = 1, so N*Ho*Wo work items.  No coordinate lies within 1e-3 of a frame border, so the mask is decided by
    exact arithmetic; values against F.grid_sample on doubles within max(4 * E_ref, 8 * 2^-24 * max|img|), E_ref
    from the same call on float32.  Seen on an MI355X: E_ref 2.3e-5, bound 9.1e-5, kernel 1.1e-5."""
    N, C, H, W, Ho, Wo = 1, 1, 37, 53, 4097, 4097
    n = wraps(N * Ho * Wo)
    img = rand(N, C, H, W, seed=10)
    g = torch.Generator(device=DEV).manual_seed(11)
    coords = torch.rand(N, Ho, Wo, 2, device=DEV, generator=g) * torch.tensor([W + 3.0, H + 3.0], device=DEV) - 2.0
    for c, border in ((0, (0.0, W - 1.0)), (1, (0.0, H - 1.0))):
        for e in border:
            near = (coords[..., c] - e).abs() < 1e-3
            coords[..., c] = torch.where(near, coords[..., c] + 0.01, coords[..., c])
    out, mask = sentinel(n), sentinel(n)
    call("raft_bilinear_sample", img.data_ptr(), coords.data_ptr(), out.data_ptr(), mask.data_ptr(), N, C, H, W, Ho, Wo)
    x, y = coords[..., 0], coords[..., 1]
    assert torch.equal(take(mask, n).view(N, Ho, Wo), ((x > 0) & (x < W - 1) & (y > 0) & (y < H - 1)).float())

    def ref(dtype):
        c = coords.to(dtype)
        grid = torch.stack([2 * c[..., 0] / (W - 1) - 1, 2 * c[..., 1] / (H - 1) - 1], -1)
        return F.grid_sample(img.to(dtype), grid, mode="bilinear", padding_mode="zeros", align_corners=True)

    ref64 = ref(torch.float64)
    bound, e_ref = measured(ref(torch.float32), ref64, 8 * EO.U * float(img.abs().max()))
    err = maxerr(take(out, n).view(N, C, Ho, Wo), ref64)
    print(f"bilinear wrap: E_ref {e_ref:.3e} bound {bound:.3e} gpu err {err:.3e}")
    assert err <= bound


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_ingest_frame_16842816(dtype):
    """B*Hp*Wp work items, float NCHW and uint8 NHWC input: the raw padded frame must equal torch's replicate
    padding, the prepped rows 2 * (x / 255) - 1 in fp64 to 3 * 2^-24 (test_gpu_layout's bound for the expression)."""
    from raft_optical_flow_amd import _lib
    B, H, W = 1, 4101, 4099
    top, bottom, left, right = 1, 2, 2, 3                       # InputPadder('sintel'): 4104 x 4104
    Hp, Wp = H + top + bottom, W + left + right
    assert Hp % 8 == 0 and Wp % 8 == 0
    n = wraps(B * Hp * Wp)
    g = torch.Generator(device=DEV).manual_seed(12)
    u8 = torch.randint(0, 256, (B, H, W, 3), device=DEV, dtype=torch.uint8, generator=g)
    nchw = u8.permute(0, 3, 1, 2).float().contiguous()
    src, tag = (u8, _lib.FRAME_U8_NHWC) if dtype == "u8" else (nchw, _lib.FRAME_F32_NCHW)
    rows, padded = sentinel(3 * n), sentinel(3 * n)
    call("raft_ingest_frame", src.data_ptr(), tag, B, H, W, 1, rows.data_ptr(), padded.data_ptr())
    want = F.pad(nchw, (left, right, top, bottom), mode="replicate")
    assert torch.equal(take(padded, 3 * n).view(B, 3, Hp, Wp), want)
    ref = (2.0 * (want.double() / 255.0) - 1.0).permute(0, 2, 3, 1).reshape(-1)
    assert maxerr(take(rows, 3 * n), ref) <= 3 * EO.U
