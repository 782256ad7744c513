"""Voxel lists that stress the kd-tree build and query of csrc/kdorder.hip, as seeded recipes (nothing here is stored: the fixture
tests/golden/kd_order.npz holds only what scikit-learn's KDTree made of these lists, tools/make_goldens_kd.py).

A recipe is (shape, order, n):
  shape  cube  a random n-subset of the smallest lattice cube that holds n voxels
         slab  the same of two z layers (coordinates heavy with duplicates)
         rod   the same of a 5 x 5 x L bar along x (all the spread in one dimension, equal keys in groups of 25) that carries a
               9^3 knot mid-way (see KNOT: without it no patch of a rod is tie-split and the device never builds its tree)
  order  random | lex (np.unique's) | rev (reverse lex) | pipe (organ pipe of lex) | saw (lex runs of 64 in random run order, as a
         first-touch list looks)
Every coordinate lies inside the valid grid of scale 1 (16 cm voxels: 0..1247, 0..1247, 0..183); only ``giveup_list`` leaves it.
NumPy only, seeded RandomState only: the same bytes under the reference interpreter and here.
"""
import zlib

import numpy as np

SCALE = 1
VOXEL = 0.16
VIS = np.array([99.84, 99.84, 14.72], dtype=np.float64)
GRID = np.array([1248, 1248, 184])
ORIGIN = np.array([400, 600, 60])           # every shape starts here: a rod of 12 000 ends at x = 879, a cube of 140 000 at z = 111
SHAPES = ("cube", "slab", "rod")
ORDERS = ("random", "lex", "rev", "pipe", "saw")
LENGTHS = (994, 995, 1920, 1921, 2048, 2049, 3840, 3841, 4096, 4097, 12000, 70000, 140000)
LONG = 12000                                # beyond: cube only, random and rev only
KD_MIN_N, KD_LEAF, KD_K, KD_SUBCAP = 994, 30, 496, 2048
N_QUERIES = 64


def recipes(n=None):
    out = []
    for m in LENGTHS if n is None else (n,):
        for shape in SHAPES:
            for order in ORDERS:
                if m > LONG and (shape != "cube" or order not in ("random", "rev")):
                    continue
                out.append((shape, order, m))
    return out


def recipe_id(r):
    return "%s-%s-%d" % r


def _seed(*parts):
    return zlib.crc32(("kd:" + ":".join(str(p) for p in parts)).encode()) & 0x7FFFFFFF


def _lattice(shape, n):
    if shape == "cube":
        s = 1
        while s ** 3 < n:
            s += 1
        dims = (s, s, s)
    elif shape == "slab":
        s = 1
        while 2 * s * s < n:
            s += 1
        dims = (s, s, 2)
    elif shape == "rod":
        dims = ((n - (KNOT ** 3 - 25 * KNOT) + 24) // 25, 5, 5)
    else:
        raise ValueError(shape)
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)   # lex order
    if shape == "rod":
        k = np.stack(np.meshgrid(*[np.arange(KNOT)] * 3, indexing="ij"), -1).reshape(-1, 3) + knot_corner(n)
        g = np.unique(np.concatenate([g, k]), axis=0)
    return g, dims


KNOT = 9   # a bare 5 x 5 bar has no tie-split patch at all (at most 16 * 25 = 400 voxels in a window: the 496-nearest cut falls outside it),
#            and the device builds a tree only for a scale that has one: a rod carries a KNOT^3 block around its axis, mid-way


def knot_corner(n):
    length = (n - (KNOT ** 3 - 25 * KNOT) + 24) // 25
    return np.array([max(0, length // 2 - KNOT // 2), 2 - KNOT // 2, 2 - KNOT // 2])


def make_list(shape, order, n):
    """-> vox [n,3] int16, distinct voxels."""
    g, dims = _lattice(shape, n)
    rs = np.random.RandomState(_seed(shape, n))
    keep = np.sort(rs.permutation(len(g))[:n])
    lex = g[keep] + ORIGIN                                             # lexsorted: np.unique(axis=0)'s order
    assert (lex >= 0).all() and (lex < GRID).all()
    ro = np.random.RandomState(_seed(shape, order, n))
    if order == "lex":
        o = np.arange(n)
    elif order == "rev":
        o = np.arange(n)[::-1]
    elif order == "pipe":
        o = np.r_[np.arange(0, n, 2), np.arange(1, n, 2)[::-1]]
    elif order == "saw":
        runs = [np.arange(a, min(a + 64, n)) for a in range(0, n, 64)]
        o = np.concatenate([runs[i] for i in ro.permutation(len(runs))])
    elif order == "random":
        o = ro.permutation(n)
    else:
        raise ValueError(order)
    return np.ascontiguousarray(lex[o].astype(np.int16))


def make_queries(vox, seed, k=N_QUERIES, box=None):
    """k key points [k,3] float32 of scale 1 whose key voxels are half uniform inside the list's box, a quarter on its faces and
    corners, a quarter up to 3 voxels outside it (the offset inside the voxel keeps the float32 point clear of its faces)."""
    rs = np.random.RandomState(_seed("q", seed))
    lo, hi = (vox.min(0).astype(np.int64), vox.max(0).astype(np.int64)) if box is None else box
    kv = np.stack([rs.randint(lo[j], hi[j] + 1, size=k) for j in range(3)], 1)
    a, b = k // 2, k // 2 + k // 4
    for i in range(a, b):                                              # faces and corners: 1 .. 3 coordinates on the box's boundary
        pin = rs.permutation(3)[:1 + (i - a) % 3]
        for j in pin:
            kv[i, j] = (lo[j], hi[j])[rs.randint(2)]
    kv[a] = lo
    kv[a + 1] = hi
    for i in range(b, k):                                              # outside: 1 .. 3 voxels beyond a face, in 1 .. 3 dimensions
        out = rs.permutation(3)[:1 + (i - b) % 3]
        for j in out:
            d = rs.randint(1, 4)
            kv[i, j] = lo[j] - d if rs.randint(2) else hi[j] + d
    assert (kv >= 0).all()
    return (kv * VOXEL - VIS + rs.uniform(0.01, 0.15, size=(k, 3))).astype(np.float32)


def key_voxels(pts, scale=SCALE):
    vs = 0.02 * (1, 8, 32)[scale]
    return ((pts.astype(np.float64) + VIS) / vs).astype(np.int32)


def recipe(r):
    """-> (vox, pts) of a recipe."""
    vox = make_list(*r)
    box = None
    if r[0] == "rod":   # (the box of the rod's knot: see KNOT)
        c = ORIGIN + knot_corner(r[2])
        box = (c, c + KNOT - 1)
    return vox, make_queries(vox, recipe_id(r), box=box)


def n_levels_of(n):
    """scikit-learn 0.24: int(log2(max(1, (n - 1) / leaf_size)) + 1), in integers."""
    if n < KD_MIN_N:
        return 0
    L = 0
    while (KD_LEAF << (L + 1)) <= n - 1:
        L += 1
    return L + 1


def top_levels_of(n):
    """The levels the device's top kernel runs before every subtree fits a workgroup's LDS (2048 voxels: KD_SUBCAP): the first
    level whose nodes hold at most 2048, a node of level L holding at most ceil(n / 2^L)."""
    L = 0
    while -(-n // (1 << L)) > KD_SUBCAP:
        L += 1
    return min(L, n_levels_of(n))


def tree_tables(vox, idx):
    """The node tables that follow from a tree's index array: node i owns idx[start, end); an inner node (one that has children in
    the table and holds at least 2 voxels) splits at m // 2; the children of a node that does not split stay (0, 0); lo / hi are the
    bounding boxes (an empty node keeps the build's initial 32767 / -32768) -> start, end [n_nodes] int32, lo, hi [n_nodes,3] int16."""
    n = len(idx)
    n_nodes = (1 << n_levels_of(n)) - 1
    start, end = np.zeros(n_nodes, np.int32), np.zeros(n_nodes, np.int32)
    lo, hi = np.full((n_nodes, 3), 32767, np.int16), np.full((n_nodes, 3), -32768, np.int16)
    if n_nodes == 0:
        return start, end, lo, hi
    end[0] = n
    for i in range(n_nodes):
        m = int(end[i]) - int(start[i])
        if 2 * i + 1 < n_nodes and m >= 2:
            start[2 * i + 1], end[2 * i + 1] = start[i], start[i] + m // 2
            start[2 * i + 2], end[2 * i + 2] = start[i] + m // 2, end[i]
    p = vox[idx]
    level, first = 0, 0
    while first < n_nodes:
        cnt = 1 << level
        s, e = start[first:first + cnt], end[first:first + cnt]
        if (e > s).all() and (s[1:] == e[:-1]).all() and s[0] == 0 and e[-1] == n:   # the usual case: the level tiles [0, n)
            lo[first:first + cnt] = np.minimum.reduceat(p, s, axis=0)
            hi[first:first + cnt] = np.maximum.reduceat(p, s, axis=0)
        else:
            for i in range(cnt):
                if e[i] > s[i]:
                    lo[first + i], hi[first + i] = p[s[i]:e[i]].min(0), p[s[i]:e[i]].max(0)
        first += cnt
        level += 1
    return start, end, lo, hi


def first_difference(got, want, start, end):
    """Where two index arrays of one tree shape part: the first differing position, the deepest node that holds it, and the
    shallowest node on the way down whose segment holds other MEMBERS (the node whose parent's selection went wrong)."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if len(bad) == 0:
        return "equal"
    p = int(bad[0])
    node, level, wrong = 0, 0, None
    while True:
        s, e = int(start[node]), int(end[node])
        if wrong is None and not np.array_equal(np.sort(got[s:e]), np.sort(want[s:e])):
            wrong = (node, level)
        c = 2 * node + 1
        if c >= len(start) or e - s < 2:
            break
        node = c if p < int(end[c]) else c + 1
        level += 1
    msg = "%d of %d positions differ, the first at %d (got %d, want %d) in node %d of level %d [%d, %d)" % (
        len(bad), len(want), p, got[p], want[p], node, level, start[node], end[node])
    if wrong is not None:
        msg += "; the first node on the way down with other members is %d of level %d" % wrong
    else:
        msg += "; every node down to it has the right members: only the order inside the leaf differs"
    return msg


# ---- the list on which the device abandons its build --------------------------------------------------------------------------
BALL_C = np.array([600, 640, 90])


def giveup_list(rod):
    """A 15^3 lattice ball (so that key voxels around its centre have tie-split patches) plus a rod 1 x 1 x ``rod`` along x through its
    centre line, the whole list sorted DESCENDING along x (stable: ties keep lex order).  Lomuto's quickselect with the last element
    as the pivot is quadratic on it.  The rod leaves the valid grid (x > 1247): the staged API takes any int16 coordinate."""
    lat = np.argwhere(np.ones((15, 15, 15), bool)) - 7
    ball = lat[(lat ** 2).sum(1) <= 49] + BALL_C
    x0 = BALL_C[0] + 8
    line = np.stack([x0 + np.arange(rod), np.full(rod, BALL_C[1]), np.full(rod, BALL_C[2])], 1)
    assert line[:, 0].max() < 32767
    v = np.concatenate([ball, line])                                   # (disjoint: the ball ends at x = 607)
    v = v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]
    return np.ascontiguousarray(v[np.argsort(-v[:, 0], kind="stable")].astype(np.int16))


def giveup_queries(k=N_QUERIES):
    rs = np.random.RandomState(_seed("giveup"))
    kv = BALL_C + rs.randint(-2, 3, size=(k, 3))
    kv[0] = BALL_C
    return (kv * VOXEL - VIS + rs.uniform(0.01, 0.15, size=(k, 3))).astype(np.float32)


# the two rod lengths, chosen with oracle.kdtree_work (tests/test_kd_order_host.py holds them to it): the root of the longer list
# spends 1.3 times its budget of 4096 passes' worth and more, the root of the shorter one 1 / 1.3 of it and less
GIVEUP_ROD, BUILT_ROD = 9400, 4800
MARGIN = 1.3


def extra_lists():
    """Lists beside the recipes that the fixture also holds scikit-learn's tree of: name -> vox."""
    return {"giveup-%d" % GIVEUP_ROD: giveup_list(GIVEUP_ROD), "giveup-%d" % BUILT_ROD: giveup_list(BUILT_ROD)}


def mixed_scales(k=N_QUERIES):
    """One map's three lists and key points: the scale-1 list is a ball of 600 voxels (brute force in the library) beside kd-sized
    lists at scales 0 (12 000, reverse lex) and 2 (994, random), each placed where the shared key points' key voxels of ITS scale
    fall (8 x and 1/4 x the scale-1 key voxels) -> ([list0, list1, list2], pts)."""
    rs = np.random.RandomState(_seed("mixed"))
    kv = BALL_C + rs.randint(-2, 3, size=(k, 3))
    kv[0] = BALL_C
    pts = (kv * VOXEL - VIS + rs.uniform(0.01, 0.15, size=(k, 3))).astype(np.float32)
    lat = np.argwhere(np.ones((15, 15, 15), bool)) - 7
    lat = lat[np.argsort((lat ** 2).sum(1), kind="stable")[:600]]
    l1 = (lat[rs.permutation(600)] + BALL_C).astype(np.int16)
    l0 = (make_list("cube", "rev", 12000).astype(np.int64) - ORIGIN - 11 + 8 * BALL_C + 4).astype(np.int16)
    l2 = (make_list("cube", "random", 994).astype(np.int64) - ORIGIN - 5 + BALL_C // 4).astype(np.int16)
    return [np.ascontiguousarray(a) for a in (l0, l1, l2)], pts
