"""tests/elementwise_oracle.py against torch and oracle/raft_oracle.py on the CPU (no GPU).

The GPU tests hold the elementwise, norm-apply, upsample, layout and caller-side kernels to that helper; here the
helper itself is held to torch's own operators in fp64 and to the reference's restatement.  The last tests record
what scipy does on exact ties in forward_interpolate: its pick is always one of the nearest sources, not always
the one with the lowest index."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_oracle as EO
from oracle import raft_oracle as O


def rng(seed):
    return np.random.default_rng(seed)


def nchw(x, h, w):
    """[B, HW, C] -> torch [B, C, H, W]"""
    b, _, c = x.shape
    return torch.from_numpy(np.ascontiguousarray(x.reshape(b, h, w, c).transpose(0, 3, 1, 2)))


def rows(t):
    """torch [B, C, H, W] -> [B, HW, C]"""
    b, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b, h * w, c).numpy()


def stats_of(x, groups):
    mean, rstd = EO.groupnorm_stats(x, groups)
    return np.stack([mean, rstd], -1)


def test_norm_apply_is_instance_norm():
    x = rng(0).normal(size=(2, 7 * 11, 6)) * 3 + np.linspace(-40, 40, 6)
    st = stats_of(x, 6)
    want = rows(F.instance_norm(nchw(x, 7, 11), eps=1e-5))
    got, mag = EO.norm_apply(x, st, 0)
    assert np.abs(got - want).max() < 1e-12
    assert np.all(mag >= np.abs(got)) and mag.shape == got.shape
    # oracle.raft_oracle's own instance norm (fp64 in, fp64 out)
    assert np.abs(got - rows(torch.from_numpy(O.instance_norm(nchw(x, 7, 11).numpy())))).max() < 1e-12


@pytest.mark.parametrize("groups", [1, 2, 12])
def test_groupnorm_stats_and_affine_apply_are_group_norm(groups):
    r = rng(groups)
    x = r.normal(size=(2, 5 * 9, 12)) * 2 + r.normal(size=12) * 30
    gamma, beta = r.normal(size=12), r.normal(size=12)
    st = stats_of(x, groups)
    want = rows(F.group_norm(nchw(x, 5, 9), groups, torch.from_numpy(gamma), torch.from_numpy(beta), eps=1e-5))
    got, _ = EO.norm_apply(x, st, 0, gamma=gamma, beta=beta)
    assert np.abs(got - want).max() < 1e-11
    plain = rows(F.group_norm(nchw(x, 5, 9), groups, eps=1e-5))
    assert np.abs(EO.norm_apply(x, st, 0)[0] - plain).max() < 1e-11
    # the statistics themselves: every channel carries its group's pair
    g = x.reshape(2, 45, groups, 12 // groups)
    assert np.allclose(st[..., 0], np.repeat(g.mean(axis=(1, 3)), 12 // groups, 1), rtol=0, atol=1e-12)
    assert np.allclose(st[..., 1], np.repeat(1 / np.sqrt(g.var(axis=(1, 3)) + 1e-5), 12 // groups, 1), rtol=1e-12)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("resid", ["none", "raw", "stats"])
def test_norm_apply_modes_are_the_residual_block_tail(mode, resid):
    """core/extractor.py's ResidualBlock: relu(x + relu(norm(y))), the shortcut raw or itself normalised."""
    r = rng(10 * mode + len(resid))
    x, s = r.normal(size=(2, 20, 4)) + 5, r.normal(size=(2, 20, 4)) - 1
    g, b, rg, rb = (r.normal(size=4) for _ in range(4))
    sx, ss = stats_of(x, 2), stats_of(s, 2)
    tx, ts = nchw(x, 4, 5), nchw(s, 4, 5)
    v = F.group_norm(tx, 2, torch.from_numpy(g), torch.from_numpy(b), eps=1e-5)
    if mode >= 1:
        v = F.relu(v)
    kw = {}
    if resid == "raw":
        v = ts + v
        kw = dict(resid=s)
    elif resid == "stats":
        v = F.group_norm(ts, 2, torch.from_numpy(rg), torch.from_numpy(rb), eps=1e-5) + v
        kw = dict(resid=s, resid_stats=ss, resid_gamma=rg, resid_beta=rb)
    if mode == 2 and resid != "none":
        v = F.relu(v)
    got, mag = EO.norm_apply(x, sx, mode, gamma=g, beta=b, **kw)
    assert np.abs(got - rows(v)).max() < 1e-11
    assert np.all(mag >= np.abs(got))


def test_upsample_and_upflow8():
    r = rng(3)
    flow = r.normal(size=(2, 2, 5, 7)) * 10
    mask = r.normal(size=(2, 576, 5, 7)) * 10
    # RAFT.upsample_flow (core/raft.py:112-142) in torch on doubles
    tf, tm = torch.from_numpy(flow), torch.from_numpy(mask)
    m = torch.softmax(tm.view(2, 1, 9, 8, 8, 5, 7), dim=2)
    uf = F.unfold(8 * tf, [3, 3], padding=1).view(2, 2, 9, 1, 1, 5, 7)
    want = torch.sum(m * uf, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(2, 2, 40, 56).numpy()
    assert np.abs(EO.upsample_flow(flow, mask) - want).max() < 1e-10
    # mask rows [B*H*W][ld] -> [B, 576, H, W]
    mrows = np.concatenate([mask.transpose(0, 2, 3, 1).reshape(-1, 576), np.full((70, 4), -7.0)], 1)
    assert np.array_equal(EO.mask_nchw(mrows, 2, 5, 7), mask)
    # upflow8: torch's interpolate on doubles == the numpy restatement on doubles
    for shape in [(2, 2, 5, 7), (1, 2, 1, 1), (1, 2, 1, 7), (1, 2, 5, 1)]:
        f = r.normal(size=shape) * 10
        assert np.abs(EO.upflow8(f) - O.upflow8(f)).max() < 1e-11, shape
    # the torch forms (for maps too large for numpy): float32 is oracle.raft_oracle's float32 arithmetic bit for
    # bit, float64 the high-precision reference
    for shape in [(2, 2, 5, 7), (1, 2, 1, 1), (1, 2, 1, 7), (1, 2, 5, 1), (1, 2, 9, 31)]:
        f = (r.normal(size=shape) * 10).astype(np.float32)
        assert np.array_equal(EO.upflow8_torch(torch.from_numpy(f), torch.float32).numpy(), O.upflow8(f)), shape
        assert np.abs(EO.upflow8_torch(torch.from_numpy(f), torch.float64).numpy() - EO.upflow8(f)).max() < 1e-11
    got = EO.upsample_flow_torch(tf, torch.from_numpy(mrows), torch.float64, chunk=32)
    assert np.abs(got.numpy() - want).max() < 1e-10
    got32 = EO.upsample_flow_torch(tf.float(), torch.from_numpy(mrows).float(), torch.float32, chunk=32)
    assert got32.dtype == torch.float32 and np.abs(got32.numpy() - want).max() < 1e-3
    # what the kernels see of their coords input
    c = (O.coords_grid(2, 5, 7) + flow.astype(np.float32)).astype(np.float32)
    assert np.array_equal(EO.flow_of_coords(c), c - O.coords_grid(2, 5, 7))
    b, e = EO.measured_bound(np.float32([1.0, np.nan, 2.5]), [1.0, 7.0, 2.0], 0.1)
    assert (b, e) == (2.0, 0.5) and EO.measured_bound([1.0], [1.0], 0.1) == (0.1, 0.0)


@pytest.mark.parametrize("hw", [(2, 2), (5, 7), (6, 9), (3, 2)])
def test_avg_pool2(hw):
    x = rng(4).normal(size=(2, 5) + hw)
    want = F.avg_pool2d(torch.from_numpy(x), 2, stride=2).numpy()
    assert np.abs(EO.avg_pool2(x) - want).max() < 1e-15
    x32 = x.astype(np.float32).transpose(0, 2, 3, 1)
    got = EO.avg_pool2_rows_fp32(x32)
    assert got.dtype == np.float32 and got.shape == (2, hw[0] // 2, hw[1] // 2, 5)
    assert np.abs(got.transpose(0, 3, 1, 2) - EO.avg_pool2(x32.transpose(0, 3, 1, 2))).max() < 3 * EO.U * np.abs(x).max()


def test_prep_images():
    r = rng(5)
    a, b = r.uniform(0, 255, size=(2, 3, 4, 5)), r.uniform(0, 255, size=(2, 3, 4, 5))
    got = EO.prep_images(a, b).reshape(4, 4, 5, 3)
    assert np.array_equal(got[1], (2 * (a[1] / 255) - 1).transpose(1, 2, 0))
    assert np.array_equal(got[2], (2 * (b[0] / 255) - 1).transpose(1, 2, 0))


def test_bilinear_sampler_is_grid_sample_and_the_restatement():
    r = rng(6)
    img = r.normal(size=(2, 3, 6, 9)).astype(np.float32)
    coords = (r.uniform(-2, 10, size=(2, 4, 5, 2))).astype(np.float32)
    coords[0, 0, 0] = (0.0, 0.0)
    coords[0, 0, 1] = (8.0, 5.0)
    coords[0, 0, 2] = (-1.0, 2.0)
    coords[0, 0, 3] = (np.nan, 1.0)
    out, m = EO.bilinear_sampler(img, coords)
    want = O.bilinear_sampler(img.astype(np.float64), coords.astype(np.float64))
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.isnan(out[0, :, 0, 3]).all()
    assert np.nanmax(np.abs(out - want)) < 1e-13
    assert out[0, 0, 0, 0] == img[0, 0, 0, 0] and out[0, 0, 0, 1] == img[0, 0, 5, 8]
    # the mask: strictly inside the frame on both axes
    x, y = coords[..., 0], coords[..., 1]
    assert np.array_equal(m[..., 0] > 0, (x > 0) & (x < 8) & (y > 0) & (y < 5))
    assert m[0, 0, 0, 0] == 0 and m[0, 0, 1, 0] == 0
    # float32: the same call in the reference's own precision
    out32, m32 = EO.bilinear_sampler(img, coords, torch.float32)
    assert out32.dtype == np.float32 and np.nanmax(np.abs(out32 - out)) < 1e-5
    assert np.array_equal(m32, m)


def continuous_flow(seed, h, w, scale=3.0):
    return (rng(seed).normal(size=(2, h, w)) * scale).astype(np.float32)


def integer_flow(seed, h, w):
    return rng(seed).integers(-3, 4, size=(2, h, w)).astype(np.float32)


@pytest.mark.parametrize("hw", [(13, 17), (24, 40)])
def test_brute_force_equals_scipy_without_ties(hw):
    f = continuous_flow(7, *hw)
    dmin, members, lowest = EO.nearest_sources(f)
    assert np.isfinite(dmin).all() and (members.sum(1) == 1).all()   # no ties on a continuous flow
    assert np.array_equal(EO.forward_interpolate_lowest(f), O.forward_interpolate(f))
    # the distance is the distance to the chosen source
    ys, xs = np.mgrid[0:hw[0], 0:hw[1]]
    x1 = (xs + f[0].astype(np.float64)).ravel()[lowest]
    y1 = (ys + f[1].astype(np.float64)).ravel()[lowest]
    assert np.array_equal(dmin, (x1 - xs.ravel()) ** 2 + (y1 - ys.ravel()) ** 2)


def test_brute_force_edges():
    z = np.zeros((2, 3, 4), np.float32)
    out_all = np.full((2, 3, 4), 100.0, np.float32)          # every source leaves the frame
    dmin, members, lowest = EO.nearest_sources(out_all)
    assert np.isinf(dmin).all() and not members.any() and (lowest == -1).all()
    assert np.array_equal(EO.forward_interpolate_lowest(out_all), z)
    one = out_all.copy()
    one[:, 1, 2] = (0.25, -0.5)                                # one valid source: its flow everywhere
    want = np.broadcast_to(np.float32([0.25, -0.5])[:, None, None], (2, 3, 4))
    assert np.array_equal(EO.forward_interpolate_lowest(one), want)
    # zero flow: sources on the frame's first row / column are not strictly inside
    _, members, lowest = EO.nearest_sources(z)
    assert not members[:, [0, 1, 2, 3, 4, 8]].any() and lowest[0] == 5
    # a NaN / Inf source never takes part
    f = continuous_flow(8, 6, 7, 1.0)
    f[0, 2, 3], f[1, 4, 4] = np.nan, np.inf
    _, members, _ = EO.nearest_sources(f)
    assert not members[:, [2 * 7 + 3, 4 * 7 + 4]].any()


def test_scipy_on_ties_picks_a_member_but_not_always_the_lowest():
    """The finding the GPU test's tie rule rests on: on an integer-valued flow many targets have several sources
    at exactly the smallest distance; scipy's cKDTree returns one of them (implementation-defined which), the
    library returns the lowest index."""
    f = integer_flow(9, 13, 17)
    dmin, members, lowest = EO.nearest_sources(f)
    tied = members.sum(1) > 1
    assert tied.sum() > 13 * 17 // 8
    got = O.forward_interpolate(f).reshape(2, -1)
    src = f.reshape(2, -1)
    # scipy's output at target t is the flow of some member of t's minimum set
    is_member = np.array([(members[t] & (src[0] == got[0, t]) & (src[1] == got[1, t])).any() for t in range(13 * 17)])
    assert is_member.all()
    # without a tie it is the only member: equal to the lowest-index rule
    low = EO.forward_interpolate_lowest(f).reshape(2, -1)
    assert np.array_equal(got[:, ~tied], low[:, ~tied])
    # with a tie it is not always the lowest index
    differs = (got != low).any(0)
    assert differs[tied].any() and not differs[~tied].any()
    print(f"tied targets: {int(tied.sum())} of {tied.size}; scipy differs from the lowest index on {int(differs.sum())}")
