"""GPU: the kd-tree build and query of csrc/kdorder.hip on adversarial voxel lists (tests/kd_lists.py), held to the CPU oracle --
which tests/test_kd_order_host.py holds to scikit-learn 0.24.2 on exactly these lists.

The tree is read back (caelo_voxmap_kd_dump) and compared element by element: the index array with the oracle's, the node tables
with what follows from that index array.  The patches -- bits and flags of all three scales -- are compared with
orc.patches_bits.  Every comparison is bit-exact."""
import time
import warnings

import numpy as np
import pytest

import kd_lists as kl

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(orc, name, lists, pts):
    """The oracle's answers for one (lists, pts), computed once per session."""
    if name not in _REF:
        trees = {}
        for s in range(3):
            if len(lists[s]) < kl.KD_MIN_N:
                continue
            same = [t for t in trees if lists[t] is lists[s]]
            if same:
                trees[s] = trees[same[0]]
            else:
                idx, n_nodes = orc.kdtree_idx(lists[s])
                trees[s] = dict(idx=idx, n_nodes=n_nodes, tables=kl.tree_tables(lists[s], idx))
        _REF[name] = dict(trees=trees, patches=[orc.patches_bits(pts, lists[s], s) for s in range(3)])
    return _REF[name]


@pytest.fixture(scope="module")
def api(engine):
    from caelo import api as _api
    return _api


def _new_map(engine, cap=None):
    from caelo.engine import VoxelMap
    return VoxelMap(engine, engine.max_points if cap is None else cap)


def _dev(engine, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _run(engine, vmap, lists, pts):
    """caelo_voxmap_from_lists + caelo_patches on ``vmap`` -> bits [K,3,64] u64, flags [K,3] u8, status."""
    vmap, st = engine.voxmap_from_lists(*[_dev(engine, a) for a in lists], vmap=vmap)
    bits, flags = engine.patches(vmap, _dev(engine, pts), None, st)
    return bits.cpu().numpy().view(np.uint64), flags.cpu().numpy(), int(st.item())


def _assert_patches(bits, flags, want, what):
    for s in range(3):
        ob, of = want["patches"][s]
        assert np.array_equal(flags[:, s], of), "%s: flags of scale %d differ at patches %s" % (what, s, np.flatnonzero(flags[:, s] != of)[:8])
        bad = np.flatnonzero((bits[:, s] != ob).any(1))
        assert len(bad) == 0, "%s: bits of scale %d differ at patches %s (flags %s)" % (what, s, bad[:8], of[bad[:8]])


def _assert_tree(engine, vmap, scale, vox, want, what):
    d = engine.kd_dump(vmap, scale)
    t = want["trees"][scale]
    n4 = int(((want["patches"][scale][1] & 4) != 0).sum())
    assert int(d["state"][4 + scale]) == 1, "%s: build state %d" % (what, d["state"][4 + scale])
    assert int(d["state"][16 + scale]) == d["n"] == len(vox) and d["n_nodes"] == t["n_nodes"] and int(d["state"][scale]) == n4, what
    assert d["top_levels"] == kl.top_levels_of(len(vox)), "%s: the top kernel runs %d levels" % (what, d["top_levels"])
    start, end, lo, hi = t["tables"]
    if not np.array_equal(d["idx"], t["idx"]):
        pytest.fail("%s: index array: %s" % (what, kl.first_difference(d["idx"], t["idx"], start, end)))
    for name, got, exp in (("start", d["start"], start), ("end", d["end"], end), ("lo", d["lo"], lo), ("hi", d["hi"], hi)):
        if not np.array_equal(got, exp):
            node = int(np.flatnonzero((got != exp).reshape(len(exp), -1).any(1))[0])
            pytest.fail("%s: %s differs first at node %d of level %d: got %s, want %s" % (
                what, name, node, int(np.log2(node + 1)), got[node], exp[node]))
    return d


@pytest.mark.parametrize("n", kl.LENGTHS)
def test_tree_and_patches_on_adversarial_lists(engine, orc, n):
    """Every recipe of this length (cube / slab / rod in random, lexsorted, reverse, organ-pipe and sawtooth order; the two longest:
    cube, random and reverse): after the patches of 64 key points the device's tree of scale 1 IS the oracle's -- state word 1, index
    array, node ranges and boxes -- and bits and flags of all three scales are the oracle's (the same list at every scale; the key
    points are scale 1's, so the other two scales see empty windows).  The lengths sit on the build's boundaries: 994 (the
    shortest list with a tree), 30 * 2^L + 1 (a level more), 2048 / 2049 and 4096 / 4097 (the top kernel starts to run levels),
    70 000 and 140 000 (its nodes fall to 32 and 16 threads)."""
    vmap = _new_map(engine)
    for r in kl.recipes(n):
        name = kl.recipe_id(r)
        vox, pts = kl.recipe(r)
        lists = [vox, vox, vox]
        want = _ref(orc, name, lists, pts)
        bits, flags, st = _run(engine, vmap, lists, pts)
        assert st == 0, name
        _assert_tree(engine, vmap, kl.SCALE, vox, want, name)
        _assert_patches(bits, flags, want, name)


def test_three_maps_behind_one_launch(engine, orc):
    """caelo_patches_many: a 70 000-voxel list, a 994-voxel list and a map whose scale-1 list is brute-force sized (600) beside
    kd-sized lists at scales 0 and 2 share one launch of each kd kernel; every map's patches and trees are those of its own
    caelo_patches call on a fresh map, and the oracle's."""
    jobs = []
    for r in (("cube", "random", 70000), ("slab", "pipe", 994)):
        vox, pts = kl.recipe(r)
        jobs.append((kl.recipe_id(r), [vox, vox, vox], pts, (kl.SCALE,)))
    lists, pts = kl.mixed_scales()
    jobs.append(("mixed", lists, pts, (0, 2)))
    wants = [_ref(orc, name, lists_, pts_) for name, lists_, pts_, _ in jobs]
    assert all(((wants[2]["patches"][s][1] & 4) != 0).any() for s in range(3)) and len(lists[1]) < kl.KD_MIN_N
    single = []
    for (name, lists_, pts_, scales), want in zip(jobs, wants):
        vm = _new_map(engine)
        bits, flags, st = _run(engine, vm, lists_, pts_)
        assert st == 0
        _assert_patches(bits, flags, want, name + " alone")
        single.append((bits, flags, [_assert_tree(engine, vm, s, lists_[s], want, name + " alone") for s in scales]))
    maps = [_new_map(engine) for _ in jobs]
    sts = [engine.voxmap_from_lists(*[_dev(engine, a) for a in lists_], vmap=vm)[1] for vm, (_, lists_, _, _) in zip(maps, jobs)]
    mbits, mflags, sts = engine.patches_many(maps, [_dev(engine, pts_) for _, _, pts_, _ in jobs], statuses=sts)
    for i, ((name, lists_, pts_, scales), want) in enumerate(zip(jobs, wants)):
        bits, flags = mbits[i].cpu().numpy().view(np.uint64), mflags[i].cpu().numpy()
        assert int(sts[i].item()) == 0
        assert np.array_equal(bits, single[i][0]) and np.array_equal(flags, single[i][1]), name
        _assert_patches(bits, flags, want, name + " of three")
        for s, alone in zip(scales, single[i][2]):
            d = _assert_tree(engine, maps[i], s, lists_[s], want, name + " of three")
            assert all(np.array_equal(d[k], alone[k]) for k in ("idx", "start", "end", "lo", "hi")), name


def test_a_map_reused_for_another_list(engine, orc):
    """List A (2049, reverse lex), list B (2048, random), A again on ONE map: each tree and result is that of a fresh map --
    caelo_voxmap_from_lists resets the state words, so the build does not take B's tree for A's ("tree already built")."""
    a, b = ("cube", "rev", 2049), ("cube", "random", 2048)
    vmap = _new_map(engine)
    for step, r in enumerate((a, b, a)):
        name = "%s (step %d)" % (kl.recipe_id(r), step)
        vox, pts = kl.recipe(r)
        want = _ref(orc, kl.recipe_id(r), [vox, vox, vox], pts)
        bits, flags, st = _run(engine, vmap, [vox, vox, vox], pts)
        fresh = _new_map(engine)
        fbits, fflags, _ = _run(engine, fresh, [vox, vox, vox], pts)
        assert st == 0 and np.array_equal(bits, fbits) and np.array_equal(flags, fflags), name
        d = _assert_tree(engine, vmap, kl.SCALE, vox, want, name)
        f = _assert_tree(engine, fresh, kl.SCALE, vox, want, name + " fresh")
        assert all(np.array_equal(d[k], f[k]) for k in ("idx", "start", "end", "lo", "hi")), name
        _assert_patches(bits, flags, want, name)


def test_abandoned_build_is_bounded_and_reported(engine, api, orc):
    """A 15^3 lattice ball with a rod along x through it, the whole list descending in x: the root's quickselect is quadratic.  With a
    rod of 4 800 the build stays inside its budget (4096 passes' worth of the root's length) and everything is the oracle's; with
    9 400 the device abandons the tree -- the call returns, the state word says 2, exactly the patches the library's order would
    have decided keep the canonical rule and flag 2 (same popcount, differing from the oracle's only in voxels at the cut distance),
    every other patch is the oracle's, GetPatchesList warns, and the next list on the same map is exact again.  The rod lengths come
    from oracle.kdtree_work (tests/test_kd_order_host.py), 1.3 times clear of the threshold on either side.  The rod reaches x = 10 007,
    beyond the valid grid (0 .. 1247): the staged API takes any int16 coordinate.  Measured on an MI355X: 102 ms for the call that
    abandons the build (upload, patches and the abandoned tree of 10 819 voxels), 0.6 s for the whole test."""
    import torch
    pts = kl.giveup_queries()
    kv = kl.key_voxels(pts)
    vmap = _new_map(engine)
    # the sibling: built, exact
    sib = kl.giveup_list(kl.BUILT_ROD)
    want = _ref(orc, "giveup-built", [sib, sib, sib], pts)
    bits, flags, st = _run(engine, vmap, [sib, sib, sib], pts)
    assert st == 0
    _assert_tree(engine, vmap, kl.SCALE, sib, want, "rod %d" % kl.BUILT_ROD)
    _assert_patches(bits, flags, want, "rod %d" % kl.BUILT_ROD)
    # the list the device gives up on
    vox = kl.giveup_list(kl.GIVEUP_ROD)
    want = _ref(orc, "giveup", [vox, vox, vox], pts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bits, flags, st = _run(engine, vmap, [vox, vox, vox], pts)
    torch.cuda.synchronize()
    print("abandoned build: %.1f ms for the call (list of %d)" % ((time.perf_counter() - t0) * 1e3, len(vox)))
    d = engine.kd_dump(vmap, kl.SCALE)
    assert st == 0 and int(d["state"][4 + kl.SCALE]) == 2 and d["n"] == len(vox)
    for s in (0, 2):
        assert np.array_equal(bits[:, s], want["patches"][s][0]) and np.array_equal(flags[:, s], want["patches"][s][1])
    ob, of = want["patches"][kl.SCALE]
    b, f = bits[:, kl.SCALE], flags[:, kl.SCALE]
    tied = (of & 4) != 0
    assert tied.sum() >= 16 and not (f & 4).any() and np.array_equal((f & 2) != 0, tied)
    assert np.array_equal(f, np.where(tied, (of & ~np.uint8(4)) | np.uint8(2), of))
    assert np.array_equal(b[~tied], ob[~tied])
    n_differ = 0
    for p in np.flatnonzero(tied):
        unpack = lambda w: np.flatnonzero(np.unpackbits(np.ascontiguousarray(w).view(np.uint8), bitorder="little"))
        got, exp = unpack(b[p]), unpack(ob[p])
        assert len(got) == len(exp), p
        d2 = np.sort(((vox.astype(np.int64) - kv[p]) ** 2).sum(1))
        cut = int(d2[kl.KD_K - 1])
        assert d2[kl.KD_K] == cut                                     # (the cut does split a class)
        lin = np.setxor1d(got, exp)
        off = np.stack([((lin >> 8) + 8) % 16 - 8, (((lin >> 4) & 15) + 8) % 16 - 8, ((lin & 15) + 8) % 16 - 8], 1)
        assert ((off ** 2).sum(1) == cut).all(), p
        n_differ += len(lin) > 0
    print("abandoned build: %d of %d tie-split patches differ from the library's order" % (n_differ, int(tied.sum())))
    with pytest.warns(RuntimeWarning, match="could not be redone"):
        api.GetPatchesList(pts, vox, vox, vox)
    # an ordinary list on the same map afterwards
    r = ("cube", "saw", 2049)
    ovox, opts = kl.recipe(r)
    want = _ref(orc, kl.recipe_id(r), [ovox, ovox, ovox], opts)
    bits, flags, st = _run(engine, vmap, [ovox, ovox, ovox], opts)
    assert st == 0
    _assert_tree(engine, vmap, kl.SCALE, ovox, want, "after the abandoned build")
    _assert_patches(bits, flags, want, "after the abandoned build")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        api.GetPatchesList(opts, ovox, ovox, ovox)


def test_list_too_long_for_the_node_table(engine):
    """30 * 2^14 + 1 voxels would need a 15th level (32 767 nodes; the table holds 16 384): refused with the capacity error.  One
    voxel fewer is accepted."""
    from caelo import _ffi
    n = 30 * (1 << 14) + 1
    big = (np.argwhere(np.ones((80, 80, 77), bool))[:n] + np.array([100, 100, 50])).astype(np.int16)
    small = kl.make_list("cube", "random", 994)
    assert len(big) == n
    vmap = _new_map(engine, n)
    with pytest.raises(_ffi.CaeloError, match=r"error -3: kd_store_lists: list too long for the node table"):
        engine.voxmap_from_lists(_dev(engine, small), _dev(engine, big), _dev(engine, small), vmap=vmap)
    _, st = engine.voxmap_from_lists(_dev(engine, small), _dev(engine, big[:-1]), _dev(engine, small), vmap=vmap)
    assert int(st.item()) == 0
