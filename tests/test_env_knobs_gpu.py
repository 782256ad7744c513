"""Every environment knob the library reads, run once: results bit-identical to the default environment.

The knobs of csrc/ are scheduling / tuning / diagnostic switches (test_library_reads_no_arithmetic_switch_from_the_environment lists
them); tools/ and the profiles measure under several of them, so a knob that changed a result would measure another computation under
the default's label.  KNOBS maps each one to the values it is run under here: child processes (the library reads its environment once
per process) run one fixed workload -- the fused extract, a plain encoder launch, a certified pipeline run -- and print a sha256 per
output; every child must reproduce the digests of this process, which runs under the default environment.  A knob csrc/ reads that is
neither in KNOBS nor covered elsewhere nor exempt fails the CPU test below.

Also here: the encoder on launches of 1 .. 257 patches against the rows of one 3072-patch launch (fewer workgroups than work queues,
the half-empty last pair of conv3, the edges of Dense(200)'s 64-row tiles).

Children run one at a time under their own time limit; after one that ended by signal, abort or timeout no further child is started."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = {
    "CAELO_S1X_SLOTS": ("1", "5", "8", "9", "1000000"),      # stage 1's grid by hand: fewer workgroups than queues, one more, all patches
    "CAELO_ENC_YIELD": ("0", "2", "7"),
    "CAELO_PIPE_STREAMS": ("1", "2"),
    "CAELO_PIPE_ENC_PRIO": ("0",),
    "CAELO_PIPE_SYSTEM_FENCES": ("1",),
    "CAELO_PIPE_VOX_STREAM": ("1", "0"),
    "CAELO_PIPE_PLAN": ("4,6,6,4",),
    "CAELO_PIPE_PACE": ("-1", "0"),
    "CAELO_CERT_THREADS": ("1", "8"),
    "CAELO_CERT_ZEROCOPY": ("0",),
    "CAELO_NO_DEDUP": ("1",),
    "CAELO_D1_WIDE_FROM": ("1",),
}
# knobs whose bit-identity case lives in another file
ELSEWHERE = {
    "CAELO_DEDUP_HASH_BITS": "tests/test_dedup_tables_gpu.py (1, 3 and 12 bits: forced hash collisions)",
    "CAELO_D1_TILE3_FROM": "tests/test_gpu_parity.py::test_dense1_tile_sizes_are_bit_identical (needs a launch of more than 16 384 rows)",
}
EXEMPT = {
    "CAELO_PIPE_VERBOSE": "prints the batch plan and stream layout to stderr; selects nothing",
    "GPU_MAX_HW_QUEUES": "the HIP runtime's own variable; the library only reads it to decide whether a voxel stream pays, which "
                         "CAELO_PIPE_VOX_STREAM overrides both ways above; tests/test_pipeline_stalls.py runs with 8",
}
# values of one knob never share a child; knobs that would make each other inert (one stream: no encoder priority, no voxel stream)
# do not either
CHILDREN = (
    {"CAELO_S1X_SLOTS": "1", "CAELO_PIPE_STREAMS": "1", "CAELO_PIPE_PACE": "-1", "CAELO_CERT_THREADS": "1"},
    {"CAELO_S1X_SLOTS": "5", "CAELO_PIPE_STREAMS": "2", "CAELO_PIPE_ENC_PRIO": "0", "CAELO_PIPE_PACE": "0"},
    {"CAELO_S1X_SLOTS": "8", "CAELO_ENC_YIELD": "0", "CAELO_PIPE_VOX_STREAM": "1", "CAELO_CERT_THREADS": "8"},
    {"CAELO_S1X_SLOTS": "9", "CAELO_ENC_YIELD": "2", "CAELO_PIPE_VOX_STREAM": "0", "CAELO_PIPE_SYSTEM_FENCES": "1"},
    {"CAELO_S1X_SLOTS": "1000000", "CAELO_ENC_YIELD": "7", "CAELO_PIPE_PLAN": "4,6,6,4"},
    {"CAELO_CERT_ZEROCOPY": "0", "CAELO_NO_DEDUP": "1", "CAELO_D1_WIDE_FROM": "1"},
)
N_FRAMES, SEED_BASE = 20, 700


def test_every_knob_of_the_library_has_a_bit_identity_case():
    src = os.path.join(REPO, "cae-lo_amd", "csrc")
    seen = set()
    for fn in os.listdir(src):
        if fn.endswith((".hip", ".inc", ".h")):
            seen |= set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', open(os.path.join(src, fn)).read()))
    assert not (set(KNOBS) & set(ELSEWHERE)) and not ((set(KNOBS) | set(ELSEWHERE)) & set(EXEMPT))
    assert seen == set(KNOBS) | set(ELSEWHERE) | set(EXEMPT), sorted(seen ^ (set(KNOBS) | set(ELSEWHERE) | set(EXEMPT)))
    assert all(EXEMPT.values()) and all(ELSEWHERE.values())
    # every value of the registry runs in exactly one child, and no child runs two values of a knob (a dict cannot)
    ran = sorted((k, v) for env in CHILDREN for k, v in env.items())
    assert ran == sorted((k, v) for k, vs in KNOBS.items() for v in vs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the workload: the same code in this process (default environment) and in every child
# ---------------------------------------------------------------------------------------------------------------------------------
def seeded_patches(n, seed):
    """n bit-packed patches [n, 64] int64 of mixed density (0.2 % .. 30 % of the voxels set)"""
    rs = np.random.RandomState(seed)
    dens = rs.choice([0.002, 0.01, 0.05, 0.3], size=n)
    return np.ascontiguousarray(np.packbits(rs.random_sample((n, 512, 8)) < dens[:, None, None], axis=2, bitorder="little").reshape(n, 512).view(np.int64))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def workload(eng, host_scans):
    import torch
    from caelo.engine import ransac_draws
    dev = eng.device
    out = {}
    scans = [torch.from_numpy(np.ascontiguousarray(pc)).to(dev) for pc in host_scans]
    for i in range(2):
        f = eng.extract(scans[i])
        out["extract %d rows" % i] = _sha(f.rows.cpu().numpy())
        out["extract %d key pixels" % i] = _sha(f.key_pixels.cpu().numpy())
    out["encode 3072 group 3"] = _sha(eng.encode(torch.from_numpy(seeded_patches(3072, 9)).to(dev), group=3).cpu().numpy())
    n = len(scans)
    draws = [ransac_draws(SEED_BASE + i) for i in range(n)]
    res = eng.pipeline(8, 3).run(scans, [torch.from_numpy(d).to(dev) for d in draws], pairs=True, certify=True, rands_host=draws)
    torch.cuda.synchronize()
    for f in ("rows", "key_pixels", "pair_idx", "inlier_mask", "result"):
        out["pipeline " + f] = _sha(getattr(res, f)[:n].cpu().numpy())
    for i, a in enumerate(res.exact):
        out["pipeline exact %d" % i] = _sha(np.ascontiguousarray(a[:n]).view(np.uint8))
    out["lane faults"] = str(eng.lane_faults())
    return out


def _child(scan_file):
    for p in (os.path.join(REPO, "cae-lo_amd"), os.path.join(REPO, "oracle")):
        sys.path.insert(0, p)
    import caelo
    caelo.configure_runtime()
    from caelo.engine import Engine
    z = np.load(scan_file)
    print("DIGESTS " + json.dumps(workload(Engine(), [z["scan%d" % i] for i in range(N_FRAMES)])))


_first_failure = None    # the first child that ended by signal, abort or timeout: no further child is started


@pytest.fixture(scope="module")
def default_digests(engine, scans, tmp_path_factory):
    """The workload in this process, and the scans in a file for the children (so that each of them need not synthesise them)."""
    host = [scans(i, quantum=1e-3) for i in range(N_FRAMES)]
    path = str(tmp_path_factory.mktemp("knobs") / "scans.npz")
    np.savez(path, **{"scan%d" % i: pc for i, pc in enumerate(host)})
    knobs = sorted(k for k in os.environ if k in KNOBS or k in ELSEWHERE)
    assert not knobs, "this process must run under the default environment, it has %s" % knobs
    want = workload(engine, host)
    assert want["lane faults"] == "0"
    return want, path


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHILDREN, ids=[" ".join("%s=%s" % kv for kv in e.items()) for e in CHILDREN])
def test_knobs_change_no_result(default_digests, env):
    global _first_failure
    want, scan_file = default_digests
    if _first_failure:
        pytest.skip("no further child after: " + _first_failure)
    label = "child " + " ".join("%s=%s" % kv for kv in env.items())
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), scan_file], env=dict(os.environ, **env), capture_output=True,
                              text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _first_failure = label + " ran into its time limit"
        pytest.fail(_first_failure)
    if proc.returncode < 0 or proc.returncode in (134, 139, 124, 137):
        _first_failure = "%s ended with %d" % (label, proc.returncode)
    assert proc.returncode == 0, "%s: exit %d\n%s" % (label, proc.returncode, proc.stderr[-3000:])
    lines = [l for l in proc.stdout.splitlines() if l.startswith("DIGESTS ")]
    assert len(lines) == 1, label
    got = json.loads(lines[0][8:])
    differing = sorted(k for k in want if got.get(k) != want[k])
    assert not differing and set(got) == set(want), "%s: %s differ from the default environment" % (label, differing)


# ---------------------------------------------------------------------------------------------------------------------------------
# encoder launch sizes
# ---------------------------------------------------------------------------------------------------------------------------------
LAUNCH_SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)


@pytest.fixture(scope="module")
def launch_patches(engine):
    import torch
    bits = seeded_patches(3072, 11)
    bits[2] = 0                                     # an empty patch
    bits[4] = -1                                    # a full one
    bits[7] = 0
    bits[7, 17] = 1 << 5                            # a single voxel
    assert sorted(set(np.unpackbits(bits[:9].view(np.uint8), axis=1).sum(axis=1).tolist()) & {0, 1, 4096}) == [0, 1, 4096]
    return torch.from_numpy(bits).to(engine.device)


def _check_launch_sizes(engine, all_bits, what):
    import torch
    want = engine.encode(all_bits, group=1)
    assert want.shape == (3072, 20)
    bad = []
    for n in LAUNCH_SIZES:
        part = all_bits[:n].contiguous()
        if not torch.equal(engine.encode(part, group=1), want[:n]):
            bad.append("%d patches" % n)
        if n % 3 == 0 and not torch.equal(engine.encode(part, group=3), want[:n].reshape(n // 3, 60)):
            bad.append("%d patches, group 3" % n)
    assert not bad, "%s: launches of %s differ from the rows of the 3072-patch launch" % (what, bad)


@pytest.mark.gpu
def test_small_encoder_launches_equal_the_large_launch(engine, launch_patches):
    """caelo_encode on the first n patches gives rows 0 .. n - 1 of the launch of all 3072 (which tests/test_weight_families_gpu.py
    holds to float64), bit for bit: n < 8 leaves work queues of stage 1 without a workgroup, an odd n gives conv3 a half-empty pair,
    n around 64 / 128 / 192 / 256 are the edges of Dense(200)'s row tiles and of the head's 16-row groups."""
    _check_launch_sizes(engine, launch_patches, "default stage 1")


@pytest.mark.gpu
def test_small_encoder_launches_equal_the_large_launch_exact_f32_stage1(engine, launch_patches):
    engine.set_encoder_reference(True)
    try:
        _check_launch_sizes(engine, launch_patches, "exact-f32 stage 1")
    finally:
        engine.set_encoder_reference(False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 9])
def test_small_launch_layers_equal_the_large_launch(engine, launch_patches, n):
    import torch
    p2, f3, _, out = (t.clone() for t in engine.encode_layers(launch_patches))
    q2, g3, _, small = engine.encode_layers(launch_patches[:n].contiguous())
    assert q2.shape == (n, 1024) and g3.shape == (n, 2048)
    assert torch.equal(q2, p2[:n]), "P2"
    assert torch.equal(g3, f3[:n]), "F3"
    assert torch.equal(small, out[:n])


if __name__ == "__main__":
    _child(sys.argv[1])
