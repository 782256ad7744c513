"""The HIP encoder and response layer on weights other than the shipped .h5 files (tests/netref64.py: seeded families and the
float64 network they are judged against).  The shipped encoder has |tanh(b1)| < 1e-3, so everything stage 1 builds around the
background vector -- the C0 border-class table, D = P1 - BG, the skipped rows, the background-output table, host tanhf against the
device tanh -- is attenuated a thousandfold there; the `biased`, `shipped_b1` and `shipped_w1neg` families run it at |bg| up to 0.38,
`sat_conv1` runs the device tanh in its overflow branch, and the reload test overwrites every derived weight buffer of a live context.

The engine of these tests is private: the session's shared engine keeps the shipped weights."""
import functools

import numpy as np
import pytest

import netref64 as nr
from test_gpu_parity import _assert_descriptors

pytestmark = pytest.mark.gpu

N_PATCHES = 70
LAYERS = ("P2", "F3", "hidden", "descriptors")

# 3 x the larger of the two stage-1 kernels' maxima that `tools/enc_layer_errors.py --family all` prints on MI355X (absolute, against
# the FLOAT64 network, on these 70 patches plus every sixth patch of the golden frame; the measured values are in
# profiles/enc_layer_errors_families.txt and in the comment behind each line) -- the convention of LAYER_BUDGET in test_gpu_parity.py.
# The descriptor bar is 1e-4 relative = 1e-5 absolute at its 0.1 floor; a family whose descriptor budget would exceed that is a defect.
FAMILY_BUDGET = {
    "shipped":      {"P2": 2.5e-06, "F3": 3.7e-06, "hidden": 5.4e-06, "descriptors": 2.7e-06},   # measured 8.11e-07 / 1.22e-06 / 1.77e-06 / 8.88e-07
    "glorot0":      {"P2": 1.1e-06, "F3": 1.5e-06, "hidden": 2.4e-06, "descriptors": 2.1e-06},   # measured 3.46e-07 / 4.90e-07 / 7.68e-07 / 6.90e-07
    "biased":       {"P2": 2.1e-06, "F3": 2.2e-06, "hidden": 4.3e-06, "descriptors": 3.9e-06},   # measured 6.85e-07 / 7.08e-07 / 1.43e-06 / 1.27e-06
    "shipped_b1":   {"P2": 2.2e-06, "F3": 3.2e-06, "hidden": 4.8e-06, "descriptors": 2.8e-06},   # measured 7.26e-07 / 1.04e-06 / 1.60e-06 / 9.32e-07
    "shipped_w1neg": {"P2": 3.6e-06, "F3": 4.0e-06, "hidden": 5.0e-06, "descriptors": 4.0e-06},   # measured 1.18e-06 / 1.31e-06 / 1.63e-06 / 1.30e-06
    "sat_conv1":    {"P2": 4.2e-06, "F3": 3.0e-06, "hidden": 5.5e-06, "descriptors": 4.1e-06},   # measured 1.38e-06 / 9.92e-07 / 1.83e-06 / 1.35e-06
}


@functools.lru_cache(maxsize=None)
def _reference(family):
    """(weights, float64 layers of the 70 edge patches): computed once per family, read-only."""
    ws = nr.encoder_family(family)
    ref = nr.encoder_layers(ws, nr.edge_patches(N_PATCHES))
    for a in ref:
        a.setflags(write=False)
    return ws, ref


def _fresh(encoder=None, respond=None):
    """A new context; ``encoder`` / ``respond`` are then the FIRST weights it ever sees (no .h5 of that kind is loaded before them)."""
    from caelo.engine import Engine, ENCODER_H5, RESPOND_H5
    e = Engine(respond_h5=None if respond is not None else RESPOND_H5, encoder_h5=None if encoder is not None else ENCODER_H5, device=0)
    if encoder is not None:
        e.set_encoder_weights(encoder)
    if respond is not None:
        e.set_respond_weights(respond)
    return e


@pytest.fixture(scope="module")
def eng(engine):   # (the session fixture first: it skips without a GPU)
    e = _fresh()
    yield e
    e.set_encoder_reference(False)


@pytest.fixture(scope="module")
def patches(eng):
    import torch
    return torch.from_numpy(nr.edge_patches(N_PATCHES).view(np.int64)).to(eng.device)


@pytest.fixture(scope="module")
def scan0(eng, scans):
    import torch
    return torch.from_numpy(scans(0)).to(eng.device)


def _layers(e, t, bd1):
    """encode_layers as float64-comparable arrays: P2, F3, tanh(Dense(200) + bias), descriptors."""
    p2, f3, pre, out = (x.cpu().numpy() for x in e.encode_layers(t))
    return p2, f3, np.tanh(pre.astype(np.float64) + np.asarray(bd1, np.float64)), out


def _raw_layers(e, t):
    return [x.cpu().numpy() for x in e.encode_layers(t)]


# ---- layers against float64, per family, on both stage-1 kernels ----------------------------------------------------------------
@pytest.mark.parametrize("family", nr.ENCODER_FAMILIES)
def test_encoder_layers_against_float64(eng, patches, family):
    ws, ref = _reference(family)
    eng.set_encoder_weights(ws)
    got = {}
    try:
        for kernel, reference in (("stage1x", False), ("stage1_f32", True)):
            eng.set_encoder_reference(reference)
            got[kernel] = _layers(eng, patches, ws[7])
    finally:
        eng.set_encoder_reference(False)
    errs = {k: {name: float(np.abs(g.astype(np.float64) - r).max()) for name, g, r in zip(LAYERS, lay, ref)} for k, lay in got.items()}
    print(family, errs)
    for kernel, lay in got.items():
        out = lay[3]
        assert np.isfinite(out).all() and all(np.isfinite(x).all() for x in lay) and np.abs(out).max() <= 1.0, (family, kernel)
        _assert_descriptors(out, ref[3])
        for name in LAYERS:
            assert errs[kernel][name] <= FAMILY_BUDGET[family][name], (family, kernel, name, errs[kernel])
    assert eng.lane_faults() == 0


# ---- exact points ---------------------------------------------------------------------------------------------------------------
def test_saturated_conv1_exact_points(eng, patches):
    """sat_conv1 drives conv1 to +-108 inside the full patch: exp(2x) overflows to inf / underflows to 0 in the device tanh, which must
    give exactly +-1 there and no NaN.  P2 of the empty patch (pure background path) and of the full patch against f32(f64 reference)
    to 2e-6; the empty patch's descriptor is the same bits from group 1 and group 3 and at any batch position."""
    import torch
    ws, ref = _reference("sat_conv1")
    eng.set_encoder_weights(ws)
    try:
        for reference in (False, True):
            eng.set_encoder_reference(reference)
            p2 = eng.encode_layers(patches)[0].cpu().numpy()
            assert not np.isnan(p2).any()
            for i in (0, 1):   # empty, full
                want = ref[0][i].astype(np.float32)
                assert np.abs(p2[i].astype(np.float64) - want).max() <= 2e-6, (reference, i, np.abs(p2[i].astype(np.float64) - want).max())
    finally:
        eng.set_encoder_reference(False)
    f = eng.encode(patches, group=1)
    g3 = eng.encode(patches[:69].contiguous(), group=3).reshape(69, 20)
    assert torch.equal(g3, f[:69])
    rs = np.random.RandomState(5)
    perm = torch.from_numpy(rs.permutation(N_PATCHES)).to(eng.device)
    assert torch.equal(eng.encode(patches[perm].contiguous(), group=1), f[perm])
    empties = torch.zeros((67, 64), dtype=torch.int64, device=eng.device)    # a batch of nothing but background
    fe = eng.encode(empties, group=1)
    assert torch.equal(fe, f[0:1].expand(67, 20))
    where = (patches != 0).any(dim=1).logical_not().nonzero().flatten().tolist()
    assert where == [0] and torch.isfinite(f).all()


# ---- the fused path on other weights ----------------------------------------------------------------------------------------------
def _own_patches(e, ff, scan):
    vm, st = e.voxelize_fast(scan, e.voxmap(slot=5))
    bits, _ = e.patches(vm, ff.key_pts.contiguous())
    assert int(st.item()) == 0
    return bits


@pytest.mark.parametrize("family", ["shipped", "shipped_b1"])
def test_fused_extract_equals_encode_of_its_own_patches(eng, scan0, family):
    """extract's descriptor columns == encode(group 3) of the frame's own patches, bit for bit, with and without de-duplication
    (`shipped` is the control: the statement holds for the path, so a failure under shipped_b1 is the weights')."""
    import torch
    eng.set_encoder_weights(_reference(family)[0])
    a = eng.extract(scan0)
    b = eng.extract(scan0, dedup=False)
    k = int(a.n_key.item())
    assert k == 1024 and int(a.status[0].item()) == 0 and int(b.status[0].item()) == 0
    assert torch.equal(a.rows[:, :63], b.rows[:, :63]) and torch.equal(a.key_pixels, b.key_pixels)
    bits = _own_patches(eng, a, scan0)
    assert len(np.unique(bits.cpu().numpy().reshape(3072, 64), axis=0)) < 3072      # de-duplication had something to do
    f = eng.encode(bits, group=3)
    assert torch.equal(f, a.features[:k])
    if family != "shipped":   # and the weights really changed the descriptors
        eng.set_encoder_weights(_reference("shipped")[0])
        assert (eng.extract(scan0).features - a.features).abs().max().item() > 1e-2


def test_encode32_on_biased_weights_against_float64(eng, scan0):
    import torch
    ws = _reference("biased")[0]
    eng.set_encoder_weights(ws)
    wd1, bd1 = eng.seeded_dense1_32()
    eng.set_encoder32_dense(wd1, bd1)
    ff = eng.extract(scan0)
    vmap, st = eng.voxelize(scan0)
    b32 = eng.patches32(vmap, ff.key_pts[::64].contiguous())                         # [16,3,512]
    pick = torch.stack([b32[i, i % 3] for i in range(16)]).contiguous()            # 16 patches, the three scales in turn
    hb = pick.cpu().numpy().view(np.uint64)
    assert int(st.item()) == 0 and hb.shape == (16, 512) and np.unpackbits(hb.view(np.uint8), axis=1).sum(axis=1).min() > 0
    got = eng.encode32(pick, group=1).cpu().numpy()
    want = nr.encoder32(ws, wd1, bd1, hb)
    assert np.isfinite(got).all() and np.abs(got).max() < 1.0
    _assert_descriptors(got, want)
    assert (want.max(axis=0) - want.min(axis=0)).min() > 1e-3


# ---- reload hygiene -----------------------------------------------------------------------------------------------------------------
def test_reloading_weights_refreshes_every_derived_buffer(engine, patches, scan0):
    """One context: shipped -> biased -> sat_conv1 -> shipped.  Every buffer the setters derive (C0 and its background-output tail,
    the split conv1 / conv2 / conv3 / Dense(200) operands, the head fragments) is allocated once and overwritten: after each switch
    the context must give the bits of a fresh context handed that family directly, and at the end its own first results."""
    import torch

    def results(e):
        out = _raw_layers(e, patches) + [e.extract(scan0).rows[:, :63].cpu().numpy()]
        e.set_encoder_reference(True)
        out.append(e.encode_layers(patches)[0].cpu().numpy())     # the f32 stage 1 reads enc_w1 / enc_b1 / enc_w2 / enc_c0 itself
        e.set_encoder_reference(False)
        return out

    live = _fresh()
    first = results(live)
    for family in ("biased", "sat_conv1", "shipped"):
        ws = _reference(family)[0]
        live.set_encoder_weights(ws)
        got = results(live)
        other = _fresh(encoder=ws)
        want = results(other)
        del other
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (family, i)
        if family != "shipped":
            assert np.abs(got[3] - first[3]).max() > 1e-2
    for i, (g, w) in enumerate(zip(got, first)):
        assert np.array_equal(g, w), i
    assert live.lane_faults() == 0
    del live
    torch.cuda.synchronize()


# ---- response layer -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring0(orc, scans):
    ring, cnt = orc.ProjectPC2SphericalRing(scans(0))
    return ring, cnt


@pytest.mark.parametrize("family", nr.RESPOND_FAMILIES)
def test_response_layer_families_bit_identical(eng, orc, ring0, family):
    """The response kernel claims the oracle's summation order (an ascending fmaf chain per output): bit identity on every family,
    `wide` with hidden units 31 binades apart; `dead` (no hidden unit fires) gives exactly relu(b2) in every pixel.  The key
    pixels selected from each response equal the oracle's; on `dead` every score is equal (zero), nothing exceeds the threshold
    and both sides refuse the frame like the reference (KeyPts.shape[0] > 50)."""
    import torch
    from caelo import api
    ring, cnt = ring0
    ws = nr.respond_family(family)
    try:
        eng.set_respond_weights(ws)
        got = eng.respond(torch.from_numpy(ring).to(eng.device)).cpu().numpy()
    finally:
        eng.set_respond_weights(nr.respond_family("shipped"))     # (extract in this module's other tests detects with the shipped layer)
    want = orc.RespondLayer(*ws).predict(ring[None, 0:64, 0:1792, 0:3])[0]
    assert got.shape == want.shape and np.array_equal(got, want)
    if family == "dead":
        assert np.array_equal(got, np.broadcast_to(np.maximum(ws[3], 0.0), got.shape)) and got.max() > 0
        with pytest.raises(AssertionError):
            orc.GetKeyPtsByAE(ring, cnt, want)
        with pytest.raises(AssertionError):
            api.GetKeyPtsByAE(ring, cnt, got)
    else:
        assert (got > 0).mean() > 0.2
        o_kp, o_kpix, _ = orc.GetKeyPtsByAE(ring, cnt, want)
        kp, kpix, _ = api.GetKeyPtsByAE(ring, cnt, got)
        assert len(o_kpix) > 50 and np.array_equal(kpix, o_kpix) and np.array_equal(kp, o_kp)


def test_setters_refuse_wrong_shapes(eng):
    ws = nr.encoder_family("glorot0")
    with pytest.raises(ValueError):
        eng.set_encoder_weights(ws[:9])
    with pytest.raises(ValueError):
        eng.set_respond_weights(ws[:4])
    bad = list(ws)
    bad[6] = np.ascontiguousarray(ws[6].T)
    with pytest.raises(ValueError):
        eng.set_encoder_weights(bad)
