"""The 32^3 path (csrc/config5.hip: k5_patches, k5_conv1pool_x3, k5_conv2_x3, k5_conv3_x3, and Dense(200) + head through
enc_dense32_head_launch) on inputs a scan never gives it: the empty and the full patch, voxels on faces, edges and corners of the
32-cube, every layer against the float64 network of tests/netref64.py, a non-zero dense_1 bias, batch sizes around the row tile and
the persistent grids, group / out_stride, and the patch gather against the set-membership rule of tests/patches32_ref.py on hand-made
voxel lists.  The references are checked on the CPU first (tests/test_weight_families_host.py).

The engine of these tests is private: the session's shared engine keeps the shipped weights."""
import ctypes as C
import functools

import numpy as np
import pytest

import netref64 as nr
import patches32_ref as pr
from test_gpu_parity import _assert_descriptors

pytestmark = pytest.mark.gpu

N_EDGE = 24
FAMILIES = ("shipped", "biased", "sat_conv1")
LAYERS = ("P1", "P2", "F3", "hidden", "descriptors")

# 3 x the maxima that `tools/enc_layer_errors.py --config5` prints on MI355X (absolute, against the FLOAT64 network, on the 24 edge
# patches, seeded dense_1 with the bias U(-0.5, 0.5); the measured values are in profiles/enc32_layer_errors_families.txt and in the
# comment behind each line) -- the convention of LAYER_BUDGET / FAMILY_BUDGET.  The descriptor bar is 1e-4 relative = 1e-5 absolute at its
# 0.1 floor; a family whose descriptor budget would exceed that is a defect.
LAYER32_BUDGET = {
    "shipped":   {"P1": 5.2e-07, "P2": 1.8e-06, "F3": 2.8e-06, "hidden": 1.6e-05, "descriptors": 8.0e-06},   # measured 1.709e-07 / 5.876e-07 / 9.055e-07 / 5.211e-06 / 2.655e-06
    "biased":    {"P1": 4.0e-07, "P2": 2.0e-06, "F3": 2.5e-06, "hidden": 7.5e-06, "descriptors": 7.7e-06},   # measured 1.331e-07 / 6.575e-07 / 8.015e-07 / 2.471e-06 / 2.549e-06
    "sat_conv1": {"P1": 5.1e-07, "P2": 2.0e-06, "F3": 2.7e-06, "hidden": 9.9e-06, "descriptors": 8.7e-06},   # measured 1.668e-07 / 6.615e-07 / 8.716e-07 / 3.280e-06 / 2.881e-06
}
# (The three conv layers sum 27, 216 and 432 terms as at 16^3 and land where their twins do -- P2 8.1e-07 / 6.9e-07 / 1.4e-06 and F3
# 1.2e-06 / 7.1e-07 / 9.9e-07 in profiles/enc_layer_errors_families.txt; Dense(200) sums 8 x the terms, 16384, and is 1.7 .. 2.9 x its twin's
# 1.8e-06 / 1.4e-06 / 1.8e-06, the square root of the length.)


@functools.lru_cache(maxsize=None)
def _dense1():
    wd1, bd1 = nr.dense1_32()
    wd1.setflags(write=False)
    bd1.setflags(write=False)
    return wd1, bd1


@functools.lru_cache(maxsize=None)
def _reference(family):
    """(weights, float64 layers of the 24 edge patches under the seeded dense_1 with its bias): once per family, read-only."""
    ws = nr.encoder_family(family)
    ref = nr.encoder32_layers(ws, *_dense1(), nr.edge_patches32(N_EDGE))
    for a in ref:
        a.setflags(write=False)
    return ws, ref


def _fresh(encoder=None):
    """A new context; ``encoder`` is then the FIRST encoder it ever sees (the shipped .h5 is not loaded before it)."""
    from caelo.engine import Engine, ENCODER_H5, RESPOND_H5
    e = Engine(respond_h5=RESPOND_H5, encoder_h5=None if encoder is not None else ENCODER_H5, device=0)
    if encoder is not None:
        e.set_encoder_weights(encoder)
    return e


@pytest.fixture(scope="module")
def eng(engine):   # (the session fixture first: it skips without a GPU)
    return _fresh()


@pytest.fixture(scope="module")
def edge(eng):
    import torch
    return torch.from_numpy(nr.edge_patches32(N_EDGE).view(np.int64)).to(eng.device)


def _use(e, family, bias=True):
    e.set_encoder_weights(_reference(family)[0])
    wd1, bd1 = _dense1()
    e.set_encoder32_dense(wd1, bd1 if bias else np.zeros(200, np.float32))


def _raw(e, t):
    return [x.cpu().numpy() for x in e.encode32_layers(t)]


@pytest.fixture(scope="module")
def base(eng, edge):
    """What the 24-patch call leaves under `biased` with the bias: P1, P2, F3, Dense(200) sums, descriptors.  Read-only."""
    _use(eng, "biased")
    out = _raw(eng, edge)
    for a in out:
        a.setflags(write=False)
    return out


def _encode32_abi(e, bits, n, group, out, stride):
    """caelo_encode32 itself, with the caller's n_patches / group / out_stride -> its return code."""
    from caelo.engine import _ptr
    ws = e._ws("encode32", int(e.lib.caelo_encode32_ws_bytes(max(n, 1))))
    return e.lib.caelo_encode32(e.ctx, _ptr(bits), n, group, _ptr(out), stride, _ptr(ws), e.stream)


# ---- layers against float64, per family -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_encoder32_layers_against_float64(eng, edge, family):
    ws, ref = _reference(family)
    bd1 = _dense1()[1]
    _use(eng, family)
    p1, p2, f3, pre, out = _raw(eng, edge)
    got = (p1, p2, f3, np.tanh(pre.astype(np.float64) + bd1.astype(np.float64)), out)
    errs = {name: float(np.abs(g.astype(np.float64) - r).max()) for name, g, r in zip(LAYERS, got, ref)}
    print(family, {k: "%.3e" % v for k, v in errs.items()})
    assert all(g.shape == r.shape for g, r in zip(got, ref))
    assert all(np.isfinite(g).all() for g in got) and np.abs(out).max() <= 1.0, family
    _assert_descriptors(out, ref[4])
    for name in LAYERS:
        assert errs[name] <= LAYER32_BUDGET[family][name], (family, name, errs)
    assert LAYER32_BUDGET[family]["descriptors"] <= 1e-5
    spread = ref[4].max(axis=0) - ref[4].min(axis=0)
    assert spread.min() >= 1e-3, (family, spread.min())
    assert eng.lane_faults() == 0


# ---- exact points ---------------------------------------------------------------------------------------------------------------------
def test_encoder32_saturated_conv1_exact_points(eng, edge):
    """sat_conv1 drives conv1 to +-108 inside the full patch: exp(2x) overflows to inf / underflows to 0 in the device tanh, which must
    give exactly +-1 there and no NaN anywhere.  P1 of the full patch's interior cells against f32(f64 reference) to 2e-6 (the bound
    test_saturated_conv1_exact_points has for P2); a batch of nothing but empty patches gives the edge batch's empty row, 67 times."""
    import torch
    ws, ref = _reference("sat_conv1")
    _use(eng, "sat_conv1")
    lay = _raw(eng, edge)
    assert not any(np.isnan(a).any() for a in lay)
    want = ref[0][1, 1:15, 1:15, 1:15].astype(np.float32)
    assert np.abs(ref[0][1, 1:15, 1:15, 1:15]).min() == 1.0            # the float64 tanh is saturated there too
    err = np.abs(lay[0][1, 1:15, 1:15, 1:15].astype(np.float64) - want).max()
    assert err <= 2e-6, err
    empties = torch.zeros((67, 512), dtype=torch.int64, device=eng.device)
    fe = eng.encode32(empties, group=1).cpu().numpy()
    assert np.array_equal(fe.view(np.uint32), np.broadcast_to(lay[4][0:1].view(np.uint32), (67, 20)))
    assert not nr.edge_patches32(N_EDGE)[0].any()


# ---- batch position and the persistent loops -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_encoder32_rows_do_not_depend_on_the_batch(eng, edge, base, n):
    """n = 1, 63 / 64 / 65 (one row tile, either side of it, one past the 64-patch grids of conv1 and conv2 -- 1024 and 512 workgroups
    of 16 and 8 items a patch) and 257 (one past the 256-patch grid of conv3: 512 workgroups, 2 items a patch); 65 and 257 leave the
    head's 16-row workgroups a ragged tail.  Every row's P1 / P2 / F3 and descriptor bits are those of the same patch in the 24-patch
    call."""
    import torch
    _use(eng, "biased")
    idx = np.random.RandomState(100 + n).permutation(np.resize(np.arange(N_EDGE), max(n, N_EDGE)))[:n]
    t = edge[torch.from_numpy(idx).to(eng.device)].contiguous()
    p1, p2, f3, _, out = _raw(eng, t)
    assert out.shape == (n, 20)
    for name, g, b in (("P1", p1, base[0]), ("P2", p2, base[1]), ("F3", f3, base[2]), ("descriptors", out, base[4])):
        same = (g.view(np.uint32).reshape(n, -1) == b[idx].view(np.uint32).reshape(n, -1)).all(axis=1)
        assert same.all(), (name, n, np.nonzero(~same)[0][:8].tolist())


# ---- group and out_stride ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2, 3])
def test_encode32_group_and_out_stride(eng, edge, base, group):
    import torch
    _use(eng, "biased")
    pick = [1, 4, 5, 11, 13, 15]
    t = edge[torch.tensor(pick, device=eng.device)].contiguous()
    stride = 20 * group + 7
    out = torch.full((6 // group, stride), 12345.0, dtype=torch.float32, device=eng.device)
    assert _encode32_abi(eng, t, 6, group, out, stride) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 20 * group:], np.full((6 // group, 7), 12345.0, np.float32))
    assert np.array_equal(got[:, :20 * group].reshape(6, 20).view(np.uint32), base[4][pick].view(np.uint32))


# ---- dense_1 reload ------------------------------------------------------------------------------------------------------------------------
def test_encoder32_dense1_bias_is_uploaded_and_replaced(eng, edge):
    """One context: zero bias -> the bias U(-0.5, 0.5) -> zero bias.  The middle result differs from the first and is the float64
    network's; the last is the first, bit for bit.  Then the conv weights change under a dense_1 that stays: the descriptors are
    those of a fresh context that saw the new weights first."""
    ws, ref = _reference("shipped")
    _use(eng, "shipped", bias=False)
    first = eng.encode32(edge).cpu().numpy()
    _use(eng, "shipped", bias=True)
    mid = eng.encode32(edge).cpu().numpy()
    assert np.abs(mid - first).max() > 1e-2
    _assert_descriptors(mid, ref[4])
    _use(eng, "shipped", bias=False)
    assert np.array_equal(eng.encode32(edge).cpu().numpy().view(np.uint32), first.view(np.uint32))
    eng.set_encoder32_dense(*_dense1())
    eng.set_encoder_weights(_reference("biased")[0])             # after set_encoder32_dense, which it must leave in place
    live = eng.encode32(edge).cpu().numpy()
    other = _fresh(encoder=_reference("biased")[0])
    other.set_encoder32_dense(*_dense1())
    want = other.encode32(edge).cpu().numpy()
    del other
    assert np.array_equal(live.view(np.uint32), want.view(np.uint32)) and np.abs(live - mid).max() > 1e-2
    _assert_descriptors(live, _reference("biased")[1][4])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_encode32_refusals_leave_the_context_usable(edge, base):
    import torch
    from caelo import _ffi
    e = _fresh(encoder=_reference("biased")[0])
    t = edge[:6].contiguous()
    with pytest.raises(_ffi.CaeloError, match="dense_1 not set"):
        e.encode32(t)
    e.set_encoder32_dense(*_dense1())
    want = e.encode32(t).cpu().numpy()
    assert np.array_equal(want.view(np.uint32), base[4][:6].view(np.uint32))
    out = torch.full((6, 20), 12345.0, dtype=torch.float32, device=e.device)
    for n, group, stride in ((0, 1, 20), (6, 0, 20), (6, 1, 19), (6, 3, 59)):
        assert _encode32_abi(e, t, n, group, out, stride) != 0 and b"bad shape" in e.lib.caelo_last_error(), (n, group, stride)
        assert np.array_equal(out.cpu().numpy(), np.full((6, 20), 12345.0, np.float32))
        assert np.array_equal(e.encode32(t).cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert e.lane_faults() == 0


# ---- the patch gather ----------------------------------------------------------------------------------------------------------------------
def _dev(e, a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a)).to(e.device)      # (a copy: the cases are read-only arrays)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def case_map(eng):
    lists, pts, tags = pr.gather_case()
    vmap, st = eng.voxmap_from_lists(*[_dev(eng, a) for a in lists])
    assert int(st.item()) == 0
    return vmap, _dev(eng, pts)


@pytest.fixture(scope="module")
def gathered(eng, case_map):
    """patches32 of every key point of the case, n_key = None: u64 [k, 3, 512], read-only."""
    vmap, pts = case_map
    bits = eng.patches32(vmap, pts).cpu().numpy().view(np.uint64)
    bits.setflags(write=False)
    return bits


def test_patches32_against_the_set_membership_rule(orc, gathered):
    """Bit for bit against tests/patches32_ref.py and against the oracle, at the three scales: key voxels in every brick phase inside
    a solid block (512 all-ones words), windows below index 0 and above the grid's top on each axis and on all three, a key point on a
    voxel face and the float32 values just below it, a key point 20 m from every voxel (512 zero words), and single voxels at offsets
    -17 / -16 / -1 / 0 / +15 / +16 on each axis (what these key points are is asserted in test_patches32_reference_and_its_case)."""
    lists, pts, tags = pr.gather_case()
    ref = pr.gather_reference()
    assert gathered.shape == ref.shape
    for s in range(3):
        bad = np.nonzero((gathered[:, s] != ref[:, s]).any(axis=1))[0]
        assert bad.size == 0, (s, [tags[i] for i in bad[:6]])
        assert np.array_equal(gathered[:, s], orc.patches32_bits(pts, lists[s], s)), s
    kind = np.array([t[0] for t in tags])
    made_for = np.array([-1 if t[1] is None else t[1] for t in tags])
    for s in range(3):
        assert (gathered[(kind == "solid") & (made_for == s), s] == ~np.uint64(0)).all()
        assert not gathered[kind == "far", s].any()
        single = gathered[(kind == "single") & (made_for == s), s]
        pop = np.unpackbits(single.view(np.uint8).reshape(len(single), -1), axis=1).sum(axis=1)
        assert pop.tolist() == [0, 1, 1, 1, 1, 0] * 3


def test_patches32_n_key_and_k_max(eng, case_map, gathered):
    """A device n_key below k_max: the rows at and past it are zero, the rows before it the bits of the n_key = None call; n_key equal
    to k_max; k_max = 1."""
    import torch
    vmap, pts = case_map
    k = pts.shape[0]
    for n in (37, k):
        n_key = torch.tensor([n], dtype=torch.int32, device=eng.device)
        got = eng.patches32(vmap, pts, n_key).cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:n], gathered[:n]) and not got[n:].any(), n
    assert gathered[37:].any()
    for i in (0, 5):      # a solid-block key point alone
        one = eng.patches32(vmap, pts[i:i + 1].contiguous()).cpu().numpy().view(np.uint64)
        assert one.shape == (1, 3, 512) and np.array_equal(one[0], gathered[i])
    one = eng.patches32(vmap, pts[5:6].contiguous(), torch.tensor([0], dtype=torch.int32, device=eng.device)).cpu().numpy()
    assert not one.any()


@pytest.mark.parametrize("ld", [4, 7])
def test_patches32_reads_key_points_at_their_row_pitch(eng, case_map, gathered, ld):
    import torch
    vmap, pts = case_map
    wide = torch.full((pts.shape[0], ld), float("nan"), dtype=torch.float32, device=eng.device)    # nothing past column 2 is read
    wide[:, 0:3] = pts
    assert wide.stride(0) == ld
    assert np.array_equal(eng.patches32(vmap, wide).cpu().numpy().view(np.uint64), gathered)


def test_patches32_of_one_voxel_set_built_both_ways(eng, orc):
    """voxelize of points at voxel centres and voxmap_from_lists of the same voxels give equal patch bits (and the reference's)."""
    pc, lists, keys = pr.both_ways_case()
    va, st_a = eng.voxelize(_dev(eng, pc), eng.voxmap(slot=6))
    vb, st_b = eng.voxmap_from_lists(*[_dev(eng, a) for a in lists], vmap=eng.voxmap(slot=7))
    t = _dev(eng, keys)
    a = eng.patches32(va, t).cpu().numpy().view(np.uint64)
    b = eng.patches32(vb, t).cpu().numpy().view(np.uint64)
    from caelo.engine import ST_FEW_VOXELS
    assert int(st_a.item()) & ~ST_FEW_VOXELS == 0 and int(st_b.item()) & ~ST_FEW_VOXELS == 0     # (scale 2 holds 8 voxels)
    assert np.array_equal(a, b)
    for s in range(3):
        assert np.array_equal(a[:, s], pr.patches32(keys, lists[s], s)), s
    assert np.unpackbits(a.view(np.uint8).reshape(8, 3, -1), axis=2).sum(axis=2).min() >= 8
