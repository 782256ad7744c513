"""The f32 CPU oracle of the two networks against an independent float64 restatement (tests/netref64.py), on weight families other
than the shipped .h5 files: untrained (glorot) nets, material conv1 biases (a background vector tanh(b1) of a few tenths, where the
HIP stage 1's background path has real work to do), a saturated conv1, dead and wide-exponent response layers.  CPU only.

The oracle is the yardstick of the GPU encoder tests; a family qualifies as a GPU test case only if the oracle itself stays within a
quarter of the project's 1e-4 bar of the f64 network on it."""
import functools
import os

import numpy as np
import pytest

import netref64 as nr
from conftest import GOLDEN

ORACLE_REL = 2.5e-5     # oracle descriptors vs f64, element-wise relative with the 0.1 floor: a quarter of the 1e-4 bar
# Activations between the layers are tanh outputs in [-1, 1], compared absolutely.  The descriptor bar is 1e-5 absolute at its 0.1
# floor; an oracle whose inner layers were further than half of that from the exact network could not stand in for it.
ORACLE_LAYER_ABS = 5e-6
N_PATCHES = 40


@functools.lru_cache(maxsize=None)
def _family(name):
    ws = nr.encoder_family(name)
    return ws, nr.encoder_layers(ws, nr.edge_patches(N_PATCHES))


def _rel(got, want):
    return (np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 0.1)).max()


@pytest.mark.parametrize("family", nr.ENCODER_FAMILIES)
def test_oracle_encoder_layers_against_float64(orc, family):
    ws, ref = _family(family)
    got = orc.PatchEncoder(ws).predict_layers(nr.edge_patches(N_PATCHES))
    errs = {k: np.abs(g.astype(np.float64) - r).max() for k, g, r in zip(("P2", "F3", "hidden", "descriptors"), got, ref)}
    rel = _rel(got[3], ref[3])
    print(family, {k: "%.2e" % v for k, v in errs.items()}, "descriptors rel %.2e" % rel)
    assert all(g.shape == r.shape for g, r in zip(got, ref))
    assert rel <= ORACLE_REL, (family, rel)
    for k in ("P2", "F3", "hidden"):
        assert errs[k] <= ORACLE_LAYER_ABS, (family, errs)


@pytest.mark.parametrize("family", nr.ENCODER_FAMILIES)
def test_encoder_families_discriminate(family):
    """Every descriptor column moves by at least 1e-2 across the patches: no family collapses the descriptors to a constant, on
    which any kernel would pass."""
    out = _family(family)[1][3]
    spread = out.max(axis=0) - out.min(axis=0)
    assert spread.min() >= 1e-2, (family, spread.min())
    assert np.abs(out).max() < 1.0


def test_family_properties():
    bits = nr.edge_patches(N_PATCHES)
    for f in nr.BACKGROUND_FAMILIES + ("sat_conv1",):
        assert np.abs(np.tanh(nr.encoder_family(f)[1].astype(np.float64))).max() >= 0.3, f
    assert not np.any(nr.encoder_family("glorot0")[1])
    assert np.abs(np.tanh(nr.encoder_family("shipped")[1].astype(np.float64))).max() < 1e-3   # why the shipped net does not test this path
    # sat_conv1: the exp of the device tanh overflows / underflows inside the full patch
    pre = nr.conv1_preact(nr.encoder_family("sat_conv1"), bits[1:2])[0]
    assert np.abs(pre[1:15, 1:15, 1:15]).min() >= 100.0
    assert (pre[1:15, 1:15, 1:15, 0::2] > 0).all() and (pre[1:15, 1:15, 1:15, 1::2] < 0).all()
    # shipped_w1neg: occupied cells (evaluated by conv1 on the device) whose pooled value is still exactly the background
    ws = nr.encoder_family("shipped_w1neg")
    occ = nr.occupied_cells(bits)
    still = (nr.pooled1(ws, bits) == np.tanh(ws[1].astype(np.float64))).all(axis=-1) & occ
    assert occ.sum() > 10000 and still.sum() >= 0.1 * occ.sum(), (occ.sum(), still.sum())
    # biased: conv2's response to the all-background patch differs between all 27 border classes
    ws = nr.encoder_family("biased")
    bgp = np.broadcast_to(np.tanh(ws[1].astype(np.float64)), (1, 8, 8, 8, 8))
    c0 = nr.conv_same(bgp, ws[2], ws[3])[0]
    cls = c0[np.ix_([0, 3, 7], [0, 3, 7], [0, 3, 7])].reshape(27, 16)
    gap = np.abs(cls[:, None] - cls[None]).max(axis=-1) + np.eye(27)
    assert gap.min() > 1e-3
    assert np.array_equal(c0[1:7, 1:7, 1:7], np.broadcast_to(c0[3, 3, 3], (6, 6, 6, 16)))   # ... and only between them


def test_oracle_encoder32_against_float64(orc):
    from caelo.engine import Engine
    ws = nr.encoder_family("biased")
    wd1, bd1 = Engine.seeded_dense1_32()
    bits = nr.random_patches32(8)
    ref = nr.encoder32(ws, wd1, bd1, bits)
    got = orc.PatchEncoder32(ws, wd1, bd1).predict_bits(bits)
    rel = _rel(got, ref)
    print("encoder32 rel %.2e" % rel)
    assert got.shape == ref.shape == (8, 20) and rel <= ORACLE_REL, rel
    assert (ref.max(axis=0) - ref.min(axis=0)).min() >= 1e-3


ENCODER32_FAMILIES = ("shipped", "biased", "sat_conv1")     # the families of tests/test_config5_gpu.py


@functools.lru_cache(maxsize=None)
def _family32(name):
    ws = nr.encoder_family(name)
    wd1, bd1 = nr.dense1_32()
    return ws, wd1, bd1, nr.encoder32_layers(ws, wd1, bd1, nr.edge_patches32(24))


def test_edge_patches32_are_the_named_patches():
    bits = nr.edge_patches32(24)
    d = nr.unpack(bits, 32)[..., 0].astype(bool)
    assert bits.shape == (24, 512) and np.array_equal(bits, nr.edge_patches32(24)) and np.array_equal(bits[:16], nr.edge_patches32(16))
    assert not d[0].any() and d[1].all()
    assert [int(x.sum()) for x in d[2:5]] == [1, 1, 2] and d[2, 0, 0, 0] and d[3, 31, 31, 31] and d[4, 0, 31, 0] and d[4, 31, 0, 31]
    planes = [d[5, 0], d[6, 31], d[7, :, 0], d[8, :, 31], d[9, :, :, 0], d[10, :, :, 31]]
    assert all(p.all() for p in planes) and all(int(d[i].sum()) == 1024 for i in range(5, 11))
    assert d[11, 1:31, 1:31, 1:31].all() and int(d[11].sum()) == 30 ** 3
    assert int(d[12].sum()) == 1 and d[12, 15, 16, 16]
    fill = d[13:].reshape(11, -1).mean(axis=1)
    assert np.all(np.abs(fill / np.tile([0.002, 0.02, 0.2], 4)[:11] - 1) < 0.5)     # (65 voxels expected at 0.002: 4 sigma = 0.5)
    wd1, bd1 = nr.dense1_32()
    from caelo.engine import Engine
    assert np.array_equal(wd1, Engine.seeded_dense1_32()[0]) and bd1.dtype == np.float32 and np.abs(bd1).min() > 0 and np.abs(bd1).max() < 0.5


def test_oracle_encoder32_on_edge_patches_with_a_dense1_bias(orc):
    """The f32 oracle and the float64 network agree on the 24 edge patches under `biased` with a NON-ZERO dense_1 bias, and the
    bias matters: the same network without it gives other descriptors."""
    ws, wd1, bd1, ref = _family32("biased")
    bits = nr.edge_patches32(24)
    got = orc.PatchEncoder32(ws, wd1, bd1).predict_bits(bits)
    rel = _rel(got, ref[4])
    print("encoder32, edge patches, bias: rel %.2e" % rel)
    assert [a.shape for a in ref] == [(24, 16, 16, 16, 8), (24, 8192), (24, 16384), (24, 200), (24, 20)]
    assert got.shape == (24, 20) and rel <= ORACLE_REL, rel
    assert np.array_equal(ref[4], nr.encoder32(ws, wd1, bd1, bits))
    assert np.abs(nr.encoder32(ws, wd1, np.zeros(200), bits[:4]) - ref[4][:4]).max() > 1e-2


@pytest.mark.parametrize("family", ENCODER32_FAMILIES)
def test_encoder32_families_discriminate(family):
    out = _family32(family)[3][4]
    spread = out.max(axis=0) - out.min(axis=0)
    print(family, "smallest column spread %.3f" % spread.min())
    assert spread.min() >= 1e-3 and np.abs(out).max() < 1.0, (family, spread.min())


def test_patches32_reference_and_its_case(orc):
    """tests/patches32_ref.py against the oracle's gather, bit for bit, on the hand-made voxel sets and key points of the GPU gather
    tests -- and the properties those key points were chosen for, stated from the reference's own output."""
    import patches32_ref as pr
    lists, pts, tags = pr.gather_case()
    ref = pr.gather_reference()
    assert ref.shape == (len(pts), 3, 512) and all(len(a) >= 496 for a in lists)
    for s in range(3):
        assert np.array_equal(orc.patches32_bits(pts, lists[s], s), ref[:, s]), s
    dense = np.stack([nr.unpack(ref[:, s], 32)[..., 0] for s in range(3)], axis=1).astype(bool)      # [k, 3, 32, 32, 32]
    kind = np.array([t[0] for t in tags])
    made_for = np.array([-1 if t[1] is None else t[1] for t in tags])
    for s in range(3):
        keys = pr.key_voxels(pts, s)
        mine = made_for == s
        solid = keys[mine & (kind == "solid")]
        assert all(sorted(solid[:, a] % 8) == list(range(8)) for a in range(3))                    # every brick phase on every axis
        assert dense[mine & (kind == "solid"), s].all()                                              # 512 all-ones words
        below = keys[mine & (kind == "below")] - 16
        assert [tuple(r) for r in (below < 0)] == [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]
        above = keys[mine & (kind == "above")] + 15 >= np.array(pr.GRID[s])
        assert [tuple(r) for r in above] == [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]
        assert dense[mine & np.isin(kind, ("below", "above")), s].reshape(8, -1).sum(axis=1).min() >= 20
        for i in np.nonzero(mine & (kind == "single"))[0]:
            axis, off = tags[i][2]
            want = np.zeros((32, 32, 32), bool)
            if -16 <= off < 16:
                idx = [0, 0, 0]
                idx[axis] = off % 32
                want[tuple(idx)] = True
            assert np.array_equal(dense[i, s], want), (s, axis, off)
        # a point on a voxel face: the float64 quotient is the integer itself, a float64 spacing below it is the voxel before
        face = {t[2]: i for i, t in enumerate(tags) if t[0] == "face"}
        q = (pts[face["hit"]].astype(np.float64) + pr.VISIBLE) / pr.SIZES[s]
        m = np.array([4992, 4992, 736]) >> (0, 3, 5)[s]
        assert np.array_equal(q, m.astype(np.float64)) and np.array_equal(keys[face["hit"]], m) and np.array_equal(keys[face["next"]], m)
        assert np.array_equal(keys[face["low"]], m - 1)
        for a in range(3):
            assert np.array_equal(keys[face["low%d" % a]], m - np.eye(3, dtype=int)[a])
        assert dense[face["hit"], s].sum() >= 20 and not np.array_equal(dense[face["hit"], s], dense[face["low"], s])
        # the far point: 20 m from every voxel of every scale
        far = int(np.nonzero(kind == "far")[0][0])
        centres = (lists[s].astype(np.float64) + 0.5) * pr.SIZES[s] - pr.VISIBLE
        assert np.linalg.norm(centres - pts[far].astype(np.float64), axis=1).min() > 20.0 and not dense[far, s].any()


def test_patches32_reference_on_the_builders_case(orc):
    import patches32_ref as pr
    pc, lists, keys = pr.both_ways_case()
    vox = orc.Voxelization(pc[:, 0:3])[6:9]
    for s in range(3):
        assert np.array_equal(np.unique(np.asarray(vox[s], np.int16), axis=0), lists[s]), s
        bits = pr.patches32(keys, lists[s], s)
        assert np.array_equal(orc.patches32_bits(keys, lists[s], s), bits) and nr.unpack(bits, 32).sum(axis=(1, 2, 3, 4)).min() >= 8


@pytest.fixture(scope="module")
def ring_image(orc, scans):
    import hashlib
    ring, _ = orc.ProjectPC2SphericalRing(scans(0))
    assert hashlib.sha256(ring.tobytes()).hexdigest() == str(np.load(os.path.join(GOLDEN, "frame_0.npz"))["ring_sha256"])
    return np.ascontiguousarray(ring[0:64, 0:1792, 0:3])


@pytest.mark.parametrize("family", nr.RESPOND_FAMILIES)
def test_oracle_response_layer_against_float64(orc, ring_image, family):
    """|oracle - f64| <= 64 u (sum |products| + |bias|) per output, u = 2^-24: the standard bound for the 27 + 32 = 59 f32
    accumulations of an output (59 u (1 + O(u)) <= 64 u), with the magnitudes taken from the f64 partial sums."""
    ws = nr.respond_family(family)
    ref, mag = nr.respond(ws, ring_image, with_magnitude=True)
    got = orc.RespondLayer(*ws).predict(ring_image[None])[0]
    err = np.abs(got.astype(np.float64) - ref)
    bound = 64 * 2.0 ** -24 * mag
    worst = (err / np.maximum(bound, 1e-300)).max()
    print(family, "worst error / bound %.3f" % worst)
    assert (err <= bound).all(), (family, worst)
    if family == "dead":
        x = np.asarray(ring_image, np.float64)[None]
        assert nr.conv_same(x, np.asarray(ws[0], np.float64), ws[1]).max() < -1.0   # no hidden unit comes near firing
        assert np.array_equal(got, np.broadcast_to(np.maximum(ws[3], 0.0), got.shape)) and got.max() > 0
    else:
        assert (ref > 0).mean() > 0.2
    if family == "wide":   # the hidden units span 31 binades
        h = np.abs(nr.conv_same(np.asarray(ring_image, np.float64)[None], np.asarray(ws[0], np.float64), ws[1])).max(axis=(0, 1, 2))
        assert h.max() / h.min() > 2.0 ** 28


def test_engine_weight_setters_check_shapes():
    from caelo.engine import Engine, ENCODER_SHAPES, RESPOND_SHAPES
    assert ENCODER_SHAPES == nr.ENCODER_SHAPES and RESPOND_SHAPES == nr.RESPOND_SHAPES
    ws = nr.encoder_family("glorot0")
    got = Engine._weight_arrays([w.astype(np.float64) for w in ws], ENCODER_SHAPES, "encoder")
    assert all(g.dtype == np.float32 and g.flags.c_contiguous and np.array_equal(g, w) for g, w in zip(got, ws))
    Engine._weight_arrays([w.ravel() for w in ws], ENCODER_SHAPES, "encoder")          # flat arrays of the right length pass
    bad = list(ws)
    bad[6] = np.ascontiguousarray(ws[6].T)
    for wrong in (bad, ws[:9], ws + [ws[9]], nr.respond_family("glorot0")):
        with pytest.raises(ValueError):
            Engine._weight_arrays(wrong, ENCODER_SHAPES, "encoder")
    with pytest.raises(ValueError):
        Engine._weight_arrays(ws[:4], RESPOND_SHAPES, "response-layer")
