"""GPU: the voxel hash tables at and beyond their capacity (csrc/voxel.hip).

A LiDAR scan fills the brick tables of a default map to a fifth at most, so no other test reaches a full table, a probe chain that
wraps the end of a table, the overflow report (CAELO_ST_MAP_FULL) or the wipe-by-list of the build that follows an overflow.  The maps
here hold 4096 points: 8192 / 2048 / 512 brick slots at the three scales, so that a probe of a full table is 2048 steps.

Clouds (deterministic; each test first checks on the CPU that its cloud has the property it claims):
  compact       3000 uniform points in an 8 m cube: fits everywhere, dense enough for the 496-nearest cut at every scale
  exactly_full  4096 points, two in each 1.28 m cell of a 64 x 32 x 1 slab: exactly 2048 scale-1 bricks, every slot of that table taken
  nearly_full   the same slab without its last 8 cells (2040 bricks)
  scattered     4096 uniform points in +-90 x +-90 x +-10 m: more scale-1 and scale-2 bricks than their tables hold
  wide1         4096 points, one in each 1.28 m cell of a 64 x 64 x 1 slab: 4096 scale-1 bricks (too many) in 256 scale-2 bricks (fit)
  wide2         1024 points, one in each 5.12 m cell of a 32 x 32 x 1 slab: 1024 scale-2 bricks (too many), 1024 scale-1 bricks (fit)
Every comparison is bitwise or set equality against the CPU oracle, or against a fresh map of the same size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_POINTS = 4096
SLOTS = (8192, 2048, 512)                      # brick slots of such a map (caelo_voxmap_create)
VIS = np.array([99.84, 99.84, 14.72])
CELLS = (0.02, 0.16, 0.64, 1.28, 5.12)         # voxel 0, brick 0 = voxel 1, voxel 2, brick 1, brick 2
ST_MAP_FULL, ST_FEW_VOXELS = 4, 8
OVERFLOWING = ("scattered", "wide1", "wide2")


def cell_counts(p):
    return [len(np.unique(np.floor((p[:, 0:3].astype(np.float64) + VIS) / d).astype(np.int64), axis=0)) for d in CELLS]


def _slab(n_cells):
    """Two points in each of the first n_cells 1.28 m cells of a 64 x 32 x 1 slab (aligned to the 5.12 m bricks), in different
    0.64 m voxels, every coordinate at least a centimetre away from any voxel face."""
    ix, iy = np.meshgrid(np.arange(64), np.arange(32), indexing="ij")
    cell = np.stack([48 + ix.ravel(), 64 + iy.ravel(), np.full(2048, 10)], axis=1)[:n_cells].astype(np.float64) * 1.28
    lo, hi = np.array([0.13, 0.21, 0.33]), np.array([0.77, 0.85, 0.97])
    pts = np.stack([cell + lo, cell + hi], axis=1).reshape(-1, 3) - VIS
    return pts.astype(np.float32)


def _cloud(name):
    rs = np.random.RandomState(0)
    if name == "compact":
        xyz = (rs.uniform(-4.0, 4.0, (3000, 3)) + np.array([10.0, 0.0, 0.0])).astype(np.float32)
    elif name == "scattered":
        xyz = rs.uniform([-90.0, -90.0, -10.0], [90.0, 90.0, 10.0], (4096, 3)).astype(np.float32)
    elif name == "exactly_full":
        xyz = _slab(2048)
    elif name == "nearly_full":
        xyz = _slab(2040)
    elif name in ("wide1", "wide2"):
        m, first, size = (64, (40, 40, 10), 1.28) if name == "wide1" else (32, (3, 3, 2), 5.12)
        ix, iy = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
        cell = np.stack([first[0] + ix.ravel(), first[1] + iy.ravel(), np.full(m * m, first[2])], axis=1).astype(np.float64) * size
        xyz = (cell + np.array([0.13, 0.21, 0.33]) - VIS).astype(np.float32)
    else:
        raise KeyError(name)
    pc = np.zeros((len(xyz), 4), dtype=np.float32)
    pc[:, 0:3] = xyz
    pc[:, 3] = 0.5
    return pc


def _sorted(a):
    a = np.asarray(a).astype(np.int32)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


@pytest.fixture(scope="module")
def api(engine):
    from caelo import api as _api
    return _api


@pytest.fixture(scope="module")
def clouds(engine, orc):
    """name -> dict(pc, dev, kp, kp_dev, lists (the oracle's AllVoxels0/1/2), sets, bits / flags (the oracle's GetPatchesList on kp)).
    Computed once, never written again.  "<name>+1": the same points rotated by one position."""
    import torch
    out = {}
    for name in ("compact", "exactly_full", "nearly_full", "scattered", "wide1", "wide2"):
        base = _cloud(name)
        for tag, pc in ((name, base), (name + "+1", np.roll(base, 1, axis=0))):
            if name in OVERFLOWING and tag != name:
                continue
            pc = np.ascontiguousarray(pc)
            kp = np.ascontiguousarray(pc[np.random.RandomState(3).choice(len(pc), 1024, replace=False), 0:3])
            d = dict(pc=pc, dev=torch.from_numpy(pc).to(engine.device), kp=kp, kp_dev=torch.from_numpy(kp).to(engine.device))
            v = orc.Voxelization(pc[:, 0:3])
            d["lists"] = [v[6], v[7], v[8]]
            d["sets"] = [_sorted(a) for a in d["lists"]]
            if name not in OVERFLOWING:
                bf = [orc.patches_bits(kp, d["lists"][s], s) for s in range(3)]
                d["bits"] = np.stack([b for b, _ in bf], axis=1)        # [1024, 3, 64] u64
                d["flags"] = np.stack([f for _, f in bf], axis=1)       # [1024, 3] u8
            out[tag] = d
    return out


def _small_map(engine):
    from caelo.engine import VoxelMap
    return VoxelMap(engine, MAX_POINTS)


def _sets(engine, vm):
    return [engine.voxmap_voxels(vm, s, capacity=SLOTS[0]) for s in range(3)]


def _patches(engine, vm, c):
    bits, flags = engine.patches(vm, c["kp_dev"])
    return bits.cpu().numpy().view(np.uint64), flags.cpu().numpy()


def _check_exact_build(engine, vm, c, what):
    """`vm` after engine.voxelize(c): the oracle's voxel sets, its lists in order, and GetPatchesList's patches and flags."""
    got = _sets(engine, vm)
    for s in range(3):
        assert np.array_equal(got[s], c["sets"][s]), "%s: exact build, voxel set of scale %d" % (what, s)
    lists = engine.voxmap_export(vm, len(c["pc"]))
    for s in range(3):
        assert np.array_equal(lists[s].cpu().numpy(), c["lists"][s]), "%s: exact build, voxel list of scale %d" % (what, s)
    engine.voxmap_order(vm, 7)
    bits, flags = _patches(engine, vm, c)
    assert np.array_equal(bits, c["bits"]), "%s: patches of the ordered map" % what
    assert np.array_equal(flags, c["flags"]), "%s: patch flags of the ordered map" % what


def _check_fast_build(engine, vm, c, fresh_patches, what):
    got = _sets(engine, vm)
    for s in range(3):
        assert np.array_equal(got[s], c["sets"][s]), "%s: fast build, voxel set of scale %d" % (what, s)
    bits, flags = _patches(engine, vm, c)
    assert np.array_equal(bits, fresh_patches[0]) and np.array_equal(flags, fresh_patches[1]), "%s: patches of the fast build" % what


def test_clouds_have_the_properties_they_claim(clouds):
    n = {k: cell_counts(c["pc"]) for k, c in clouds.items()}
    print("occupied cells at", CELLS, n)
    for k in ("compact", "compact+1"):
        assert n[k][0] >= 496 and n[k][1] >= 496 and n[k][2] >= 496
        assert n[k][1] <= SLOTS[0] // 2 and n[k][3] <= SLOTS[1] // 2 and n[k][4] <= SLOTS[2] // 2
    for k in ("exactly_full", "exactly_full+1"):
        assert n[k] == [4096, 4096, 4096, SLOTS[1], 16 * 8]         # every slot of the scale-1 brick table, and no brick too many
    for k in ("nearly_full", "nearly_full+1"):
        assert n[k] == [4080, 4080, 4080, SLOTS[1] - 8, 16 * 8]
    assert n["scattered"][1] <= SLOTS[0] and n["scattered"][3] > SLOTS[1] and n["scattered"][4] > SLOTS[2]
    assert n["wide1"] == [4096, 4096, 4096, 4096, 256] and n["wide1"][3] > SLOTS[1] and n["wide1"][4] <= SLOTS[2]      # scale 1 alone
    assert n["wide2"] == [1024] * 5 and n["wide2"][3] <= SLOTS[1] and n["wide2"][4] > SLOTS[2]                        # scale 2 alone
    for k, c in clouds.items():
        assert len(c["pc"]) <= MAX_POINTS
        # the oracle's sets are those cells (no point lies on a voxel face)
        assert [len(a) for a in c["sets"]] == n[k][0:3], k


@pytest.mark.parametrize("name", ["compact", "exactly_full", "nearly_full", "compact+1", "exactly_full+1", "nearly_full+1"])
def test_fitting_cloud_in_a_small_map(engine, orc, clouds, name):
    """Both builds of a cloud that fits -- at load 1.0 of the scale-1 brick table for exactly_full -- give status 0 and the oracle's
    voxel sets; the exact build its lists in order and, ordered, GetPatchesList's patches with their flags; the fast build's patches
    are those of the exact build's (unordered) map."""
    c = clouds[name]
    vm_exact, vm_fast = _small_map(engine), _small_map(engine)
    _, st = engine.voxelize(c["dev"], vm_exact)
    assert int(st.item()) == 0
    canonical = _patches(engine, vm_exact, c)       # before the order is recorded: the canonical rule on the voxel SETS
    _check_exact_build(engine, vm_exact, c, name)
    _, st = engine.voxelize_fast(c["dev"], vm_fast)
    assert int(st.item()) == 0
    _check_fast_build(engine, vm_fast, c, canonical, name)
    # and once more on the same maps: the fast build wipes its own bricks by their lists, the exact build clears whole tables
    _, st = engine.voxelize_fast(c["dev"], vm_fast)
    assert int(st.item()) == 0
    _check_fast_build(engine, vm_fast, c, canonical, name + " (second build)")


def test_lookups_in_a_full_table_end_on_the_probe_bound(engine, clouds):
    """exactly_full leaves no empty slot in the scale-1 brick table: a lookup of an absent brick (most of the 125 of a ball cube around
    a key point of a one-brick-thick slab) can only end on the probe bound of table_find, 2048 steps.  At most 1024 x 125 x 2048 =
    2.6e8 dependent loads from a 16 KB table: milliseconds; a lookup that did not end would never finish.  The bound is a second."""
    import torch
    c = clouds["exactly_full"]
    vm = _small_map(engine)
    _, st = engine.voxelize_fast(c["dev"], vm)
    engine.patches(vm, c["kp_dev"])                  # (first launch: code load)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    bits, flags = engine.patches(vm, c["kp_dev"])
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    print("exactly_full: patch gather of 1024 key points in %.3f ms" % ms)
    assert int(st.item()) == 0 and ms < 1000.0
    # no patch of the slab reaches the 496-nearest cut, so the patches of the voxel SETS are GetPatchesList's
    assert not c["flags"].any()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), c["bits"]) and np.array_equal(flags.cpu().numpy(), c["flags"])


def _overflow(engine, vm, c, kind):
    """One overflowing call on `vm` -> its status word."""
    import torch
    if kind == "voxelize":
        return int(engine.voxelize(c["dev"], vm)[1].item())
    if kind == "voxelize_fast":
        return int(engine.voxelize_fast(c["dev"], vm)[1].item())
    if kind == "from_lists":
        a = [torch.from_numpy(np.ascontiguousarray(l)).to(engine.device) for l in c["lists"]]
        return int(engine.voxmap_from_lists(a[0], a[1], a[2], vm)[1].item())
    assert kind == "extract"
    return int(engine.extract(c["dev"], vmap=vm, key_pts=c["kp_dev"]).status[0].item())


@pytest.fixture(scope="module")
def fresh(engine, clouds):
    """compact through fresh maps: the canonical patches of the voxel sets, and the rows of extract(key_pts=...)."""
    c = clouds["compact"]
    vm = _small_map(engine)
    engine.voxelize_fast(c["dev"], vm)
    canonical = _patches(engine, vm, c)
    vm2 = _small_map(engine)
    ff = engine.extract(c["dev"], vmap=vm2, key_pts=c["kp_dev"])
    assert int(ff.status[0].item()) == 0
    return dict(canonical=canonical, rows=ff.rows.cpu().numpy().view(np.uint32).copy(), flags=ff.flags.cpu().numpy().copy())


@pytest.fixture(scope="module")
def shared_map(engine):
    """ONE map for every overflow / recovery case below: whatever an overflow leaves behind meets the next case too."""
    return _small_map(engine)


def test_overflowing_cloud_raises_through_the_api(engine, api, clouds, monkeypatch):
    from caelo import _ffi
    monkeypatch.setattr(engine, "max_points", MAX_POINTS)      # the API's map of the current stream then has 4096 points
    assert api.default_engine() is engine
    with pytest.raises(_ffi.CaeloError, match="voxel map overflow"):
        api.Voxelization(clouds["scattered"]["pc"][:, 0:3])
    v = api.Voxelization(clouds["compact"]["pc"][:, 0:3])        # the same map, next call
    for s in range(3):
        assert np.array_equal(v[6 + s], clouds["compact"]["lists"][s])


@pytest.mark.parametrize("follow", ["fast", "exact", "extract"])
@pytest.mark.parametrize("kind", ["voxelize_fast", "voxelize", "from_lists", "extract"])
def test_map_is_reusable_after_an_overflow(engine, clouds, fresh, shared_map, kind, follow):
    """scattered overflows the scale-1 and scale-2 brick tables: every entry point reports CAELO_ST_MAP_FULL (nothing is asserted
    about that frame's voxels or rows).  The same map then takes compact and gives the bits of a fresh map -- through the fast build
    (which wipes the overflowed build's bricks by their lists, k_vox_clear_lists, when that was a fast build too), the exact build,
    and the fused extract."""
    c, bad, vm = clouds["compact"], clouds["scattered"], shared_map
    st = _overflow(engine, vm, bad, kind)
    assert st & ST_MAP_FULL, "%s: status %d" % (kind, st)
    what = "%s overflow, then %s" % (kind, follow)
    if follow == "fast":
        _, st = engine.voxelize_fast(c["dev"], vm)
        assert int(st.item()) == 0, what
        _check_fast_build(engine, vm, c, fresh["canonical"], what)
    elif follow == "exact":
        _, st = engine.voxelize(c["dev"], vm)
        assert int(st.item()) == 0, what
        _check_exact_build(engine, vm, c, what)
    ff = engine.extract(c["dev"], vmap=vm, key_pts=c["kp_dev"])
    assert int(ff.status[0].item()) == 0, what
    assert np.array_equal(ff.rows.cpu().numpy().view(np.uint32), fresh["rows"]), what + ": rows of extract(key_pts=...)"
    assert np.array_equal(ff.flags.cpu().numpy(), fresh["flags"]), what
    got = _sets(engine, vm)
    for s in range(3):
        assert np.array_equal(got[s], c["sets"][s]), "%s: voxel set of scale %d after extract" % (what, s)


@pytest.mark.parametrize("kind", ["voxelize_fast", "voxelize", "from_lists"])
@pytest.mark.parametrize("name", ["wide1", "wide2"])
def test_each_brick_table_reports_its_own_overflow(engine, clouds, fresh, shared_map, name, kind):
    """wide1 overflows the scale-1 brick table alone, wide2 the scale-2 table alone: each place that can fail to insert a brick has
    to raise the status bit itself.  The map then takes compact like a fresh one."""
    c, vm = clouds["compact"], shared_map
    st = _overflow(engine, vm, clouds[name], kind)
    assert st & ST_MAP_FULL, "%s, %s: status %d" % (name, kind, st)
    _, st = engine.voxelize_fast(c["dev"], vm)
    assert int(st.item()) == 0
    _check_fast_build(engine, vm, c, fresh["canonical"], "%s %s overflow, then fast" % (name, kind))


def test_overflowing_frames_inside_pipeline_batches(engine, clouds):
    """Frames that overflow their map share batches with frames that fit, and the ring of maps wraps, so that a map that overflowed is
    reused by a fitting frame: every fitting frame equals its single extract through a fresh small map."""
    import torch
    from caelo.engine import Pipeline
    order = ["compact", "scattered", "exactly_full", "compact", "compact", "scattered", "compact", "compact", "compact", "exactly_full"]
    pipe = Pipeline(engine, 4, 2, max_points=MAX_POINTS)
    out = pipe.run([clouds[n]["dev"] for n in order], pairs=False, keypts=[clouds[n]["kp_dev"] for n in order])
    torch.cuda.synchronize()
    status = out.status.cpu().numpy()
    rows = out.rows.cpu().numpy().view(np.uint32)
    flags = out.flags.cpu().numpy()
    want = {}
    for n in ("compact", "exactly_full"):
        vm = _small_map(engine)
        ff = engine.extract(clouds[n]["dev"], vmap=vm, key_pts=clouds[n]["kp_dev"])
        want[n] = (ff.rows.cpu().numpy().view(np.uint32), ff.flags.cpu().numpy(), ff.status.cpu().numpy())
        assert int(want[n][2][0]) == 0
    for i, n in enumerate(order):
        if n == "scattered":
            assert status[i, 0] & ST_MAP_FULL, "frame %d: status %d" % (i, status[i, 0])
            continue
        assert np.array_equal(status[i], want[n][2]), "frame %d (%s): status %s" % (i, n, status[i])
        assert np.array_equal(rows[i], want[n][0]), "frame %d (%s): rows" % (i, n)
        assert np.array_equal(flags[i], want[n][1]), "frame %d (%s): flags" % (i, n)
    assert (out.n_key.cpu().numpy() == 1024).all()
    assert engine.lane_faults() == 0
