"""The host side of descriptors up to 256 wide: the descriptor files of caelo.keysources, the workspace sizes of the C ABI, the
argument checks of run_sequence.py --desc-dir and the golden tool.  No GPU needed."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO


def test_descriptor_files_round_trip_and_errors(tmp_path):
    from caelo import keysources
    rs = np.random.RandomState(2)
    for k, dim in [(1, 1), (50, 32), (700, 128), (1024, 256)]:
        d = rs.uniform(-1, 1, (k, dim)).astype(np.float32)
        p = keysources.write_descriptors(keysources.desc_path(str(tmp_path / "d"), 7), d)
        assert p.endswith("000007.bin") and os.path.getsize(p) == 4 * k * dim
        back = keysources.read_descriptors(p, dim)
        assert back.dtype == np.float32 and np.array_equal(back, d)
    p = keysources.write_descriptors(str(tmp_path / "x.bin"), np.zeros((10, 128)))       # (float64 in: float32 on disk)
    assert os.path.getsize(p) == 10 * 128 * 4
    with pytest.raises(ValueError, match=r"x\.bin: 5120 bytes do not make rows of 96 float32 \(384 bytes each\)"):
        keysources.read_descriptors(p, 96)
    with pytest.raises(FileNotFoundError, match="000003.bin"):
        keysources.read_descriptors(keysources.desc_path(str(tmp_path / "d"), 3), 128)
    with pytest.raises(ValueError, match="x.bin"):
        keysources.read_descriptors(p, 0)
    with pytest.raises(ValueError, match="y.bin"):
        keysources.write_descriptors(str(tmp_path / "y.bin"), np.zeros(12))
    keysources.write_descriptors(str(tmp_path / "big.bin"), np.zeros((1025, 8)))
    with pytest.raises(ValueError, match="staged API"):
        keysources.read_descriptors(str(tmp_path / "big.bin"), 8)
    # the rows still end at 60 columns, and the message says where wider descriptors go
    with pytest.raises(ValueError, match="desc="):
        keysources.rows_from_features(np.zeros((5, 3)), np.zeros((5, 128)))


def test_match_workspace_sizes_and_the_abi():
    from caelo import _ffi
    lib = _ffi.load()
    assert lib.caelo_abi_version() == 6
    header = open(os.path.join(REPO, "include", "caelo.h")).read()
    for name in ("caelo_match_ws_bytes_dim", "caelo_register_pairs_desc", "caelo_register_pairs_ws_bytes_dim"):
        assert hasattr(lib, name) and name + "(" in header
    for k in (1, 17, 1000, 1024, 2050):
        old = lib.caelo_match_ws_bytes(k)
        sizes = [lib.caelo_match_ws_bytes_dim(k, dim) for dim in range(1, 257)]
        assert all(s == old for s in sizes[:64])                          # dim <= 64: exactly the old function
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))              # never shrinks as dim grows
        assert sizes[64] > old and sizes[255] > sizes[127]                # one more operand image per K = 64 block
        # 256 B of counters + nb images of 4 KiB per 16-row tile + one float per row; the norm slots push 255 and 256 into a fifth block
        kp = (k + 15) // 16 * 16
        for dim, nb in ((65, 2), (126, 2), (127, 3), (190, 3), (191, 4), (254, 4), (255, 5), (256, 5)):
            assert sizes[dim - 1] == 256 + kp // 16 * nb * 4096 + 4 * kp
    for dim in (1, 60, 64):
        assert lib.caelo_register_pairs_ws_bytes_dim(12, dim) == lib.caelo_register_pairs_ws_bytes(12)
    assert lib.caelo_register_pairs_ws_bytes_dim(12, 256) >= 8 * (lib.caelo_match_ws_bytes_dim(1024, 256) + lib.caelo_ransac_ws_bytes())
    assert lib.caelo_register_pairs_ws_bytes_dim(-1, 128) == 0
    # null descriptors and widths outside [1, 256] are refused before anything else is looked at
    ctx = _ffi.c_vp(1)
    for desc, ld, dim, word in ((None, 128, 128, "null"), (_ffi.c_vp(16), 257, 257, "dim"), (_ffi.c_vp(16), 64, 0, "dim"), (_ffi.c_vp(16), 100, 128, "ld_desc")):
        rc = lib.caelo_register_pairs_desc(ctx, None, 1, None, None, 0, None, None, None, None, None, None, None, desc, ld, dim)
        assert rc != 0 and word in lib.caelo_last_error().decode()


def test_desc_dir_arguments(tmp_path):
    from caelo import keysources
    d = str(tmp_path / "desc")
    with pytest.raises(ValueError, match=r"--desc-dim.*frame 0"):
        keysources.DescSource(d, None, "usip", str(tmp_path / "kp"))
    with pytest.raises(ValueError, match=r"frame 0"):
        keysources.DescSource(d, 257, "usip", str(tmp_path / "kp"))
    with pytest.raises(ValueError, match=r"key points of frame 0.*--keypts-source"):
        keysources.DescSource(d, 128)                                     # no key point source: nothing is detected here
    with pytest.raises(ValueError, match=r"--keypts-dir.*frame 0"):
        keysources.DescSource(d, 128, "usip")
    with pytest.raises(ValueError, match="exclude"):
        keysources.DescSource(d, 128, "usip", str(tmp_path / "kp"), str(tmp_path / "Features"))
    rs = np.random.RandomState(4)
    for f, (k, kd) in enumerate([(40, 40), (33, 33), (50, 49)]):
        keysources.write_usip(keysources.keypts_path(str(tmp_path / "kp"), f), rs.uniform(-30, 30, (k, 3)))
        keysources.write_descriptors(keysources.desc_path(d, f), rs.uniform(-1, 1, (kd, 128)))
    src = keysources.DescSource(d, 128, "usip", str(tmp_path / "kp"))
    assert src.n_frames() == 3
    pts, desc = src.frame(1)
    assert pts.shape == (33, 3) and desc.shape == (33, 128) and np.array_equal(pts, keysources.read_usip(keysources.keypts_path(str(tmp_path / "kp"), 1)))
    with pytest.raises(ValueError, match=r"frame 2: 50 key points but 49 descriptors of width 128 in .*000002\.bin"):
        src.frame(2)
    with pytest.raises(ValueError, match=r"frame 0: .*000000\.bin: 20480 bytes do not make rows of 96"):
        keysources.DescSource(d, 96, "usip", str(tmp_path / "kp")).frame(0)
    # the key points of --features-from files; their Features are not looked at
    feats = str(tmp_path / "seq" / "Features")
    keysources.save_features(str(tmp_path / "seq" / "velodyne" / "000000.bin"), rs.uniform(-30, 30, (40, 3)).astype(np.float32), np.zeros((40, 60), np.float32))
    pts, desc = keysources.DescSource(d, 128, features_from=feats).frame(0)
    assert pts.shape == (40, 3) and pts.dtype == np.float32 and desc.shape == (40, 128)
    # the command line refuses the same things with the same words, and several GPUs, before any device work
    script = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")
    for extra, word in ((["--desc-dir", d], b"--desc-dim"), (["--desc-dir", d, "--desc-dim", "128"], b"--keypts-source"),
                        (["--desc-dim", "128"], b"--desc-dir"),
                        (["--desc-dir", d, "--desc-dim", "128", "--keypts-source", "usip", "--keypts-dir", str(tmp_path / "kp"), "--gpus", "2"], b"one GPU")):
        r = subprocess.run([sys.executable, script, "--out", str(tmp_path / "p.txt")] + extra, capture_output=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, r.stderr.decode()[-500:]


def test_golden_tool_imports_without_the_reference(orc):
    """tools/make_goldens_wide.py touches the reference under __main__ only; its generator reproduces the golden's inputs, and the
    oracle under this interpreter's NumPy reproduces the golden's results (the pairs do not hinge on a rank-deficient sample, whose
    score depends on the LAPACK build: see the tool's note)."""
    path = os.path.join(REPO, "tools", "make_goldens_wide.py")
    text = open(path).read()
    head = text[:text.index("def main():")]
    assert not re.search(r"^\s*(import|from)\s+(Match|Voxel|Transformations|oracle)\b", head, re.M) and "sys.path.insert" not in head
    before = set(sys.modules)
    spec = importlib.util.spec_from_file_location("make_goldens_wide", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert not {"Match", "cupy", "mayavi"} & (set(sys.modules) - before)
    g = np.load(os.path.join(GOLDEN, "wide_desc.npz"))
    assert int(g["dim"]) == mod.DIM == 128 and os.path.getsize(os.path.join(GOLDEN, "wide_desc.npz")) < 512 * 1024
    for name, (K, outliers, dn, pn, seed, rseed) in mod.PAIRS.items():
        p0, f0, p1, f1, perm, R, T = mod.make_pair(K, outliers, dn, pn, seed)
        assert K in (50, 256) and int(g[name + "_seed"]) == rseed
        for key, arr in (("_p0", p0), ("_f0", f0), ("_p1", p1), ("_f1", f1)):
            assert np.array_equal(g[name + key], arr), name + key
        oR, oT, ok, i0, i1, thr = orc.SolveRelativePose(p0, f0, None, p1, f1, None, rng=np.random.RandomState(rseed))
        assert ok == bool(g[name + "_ok"]) and thr == float(g[name + "_thr"]) and np.array_equal(orc.match(f0, f1)[0], g[name + "_pair_idx"])
        assert np.array_equal(i0, g[name + "_idx0"]) and np.array_equal(i1, g[name + "_idx1"])
        assert np.abs(oR - g[name + "_R"]).max() <= 1e-5 and np.abs(oT - g[name + "_T"]).max() <= 1e-4
