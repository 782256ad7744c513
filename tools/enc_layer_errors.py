"""Per-layer error of the HIP encoder against the f32 CPU oracle (and of the oracle against an f64 evaluation of the same
network): max |difference| after pool2 (P2), after conv3 (F3), of the Dense(200) pre-activations and of the descriptors,
on every patch of the quantised golden frame.  `CAELO_ENC_S1=f32 python tools/enc_layer_errors.py` measures round 2's
f32-input stage 1 for comparison.  The budget table of tests/test_gpu_parity.py::test_encoder_layer_error_budget is
3 x what this prints for the default kernels.

`--family NAME` (repeatable; `--family all`): the same layers under one of the seeded weight families of tests/netref64.py, judged
against the FLOAT64 network instead of the oracle, for both stage-1 kernels, on the 70 edge patches of the family tests plus every
sixth patch of the golden frame.  FAMILY_BUDGET of tests/test_weight_families_gpu.py is 3 x the larger of the two kernels' lines.

`--activations`: the models of tests/test_encoder_activations_gpu.py (tests/netref64_act.py MODELS: the trained relu / linear fixture
and seeded families under relu / linear, relu / tanh and tanh / linear) on that test's 582 patches, for both stage-1 kernels, against
the FLOAT64 network -- and, first, what the plain float32 NumPy restatement costs on the same patches: the test's per-layer bars are
4 x those lines, its descriptor bar is 1e-4 relative.  profiles/enc_layer_errors_activations.txt is this output.

`--config5`: the 32^3 encoder (csrc/config5.hip) layer by layer -- P1, P2, F3, tanh(Dense(200)), descriptors -- under the `shipped`,
`biased` and `sat_conv1` families with the seeded dense_1 and a non-zero bias, on the 24 edge patches of tests/test_config5_gpu.py,
against the FLOAT64 network.  LAYER32_BUDGET of that test is 3 x these lines; profiles/enc32_layer_errors_families.txt is this output."""
import argparse, os, sys
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd")); sys.path.insert(0, os.path.join(REPO, "oracle"))
import caelo; caelo.configure_runtime()
import oracle as orc
from caelo.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--family", action="append", default=[])
ap.add_argument("--activations", action="store_true")
ap.add_argument("--config5", action="store_true")
args = ap.parse_args()
eng = Engine(device=0)
golden_bits = np.ascontiguousarray(np.load(os.path.join(REPO, "tests", "golden", "frame_q0.npz"))["patch_bits"].reshape(-1, 64))


def report(layers, bd1, ref, hidden=np.tanh, hidden_name="tanh"):
    p2, f3, pre, out = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in layers)
    h = hidden(pre.astype(np.float64) + np.asarray(bd1, np.float64)) if bd1 is not None else pre
    for name, a, b in (("P2", p2, ref[0]), ("F3", f3, ref[1]), ("%s(Dense(200))" % hidden_name, h, ref[2]), ("descriptors", out, ref[3])):
        d = np.abs(a.astype(np.float64) - b)
        print("%-18s max abs %.3e   mean abs %.3e   element-wise rel (floor 0.1) %.3e" % (name, d.max(), d.mean(), (d / np.maximum(np.abs(b), 0.1)).max()))


if args.activations:
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import netref64_act as na
    bits = na.test_patches()
    t = torch.from_numpy(bits.view(np.int64)).to(eng.device)
    with tempfile.TemporaryDirectory() as tmp:
        for name, _, _ in na.MODELS:
            ws, acts = na.model(name, tmp)
            ref, _ = na.encoder_layers(ws, bits, acts)
            f32, _ = na.encoder_layers(ws, bits, acts, np.float32)
            bounds = na.range_bounds(ws, acts)
            print("model %s, hidden %s, code %s, %d patches; range bounds %s" % (name, acts[0], acts[1], len(bits), " ".join("%.4g" % b for b in bounds)))
            print("  plain float32 NumPy restatement, against float64")
            report(f32, None, ref, hidden_name=acts[0])
            eng.set_encoder_weights(ws, activations=acts)
            for reference in (False, True):
                eng.set_encoder_reference(reference)
                layers = eng.encode_layers(t)
                torch.cuda.synchronize()
                print("  stage 1 = %s, against float64" % ("k_enc_stage1 (f32)" if reference else "k_enc_stage1x"))
                report(layers, ws[7], ref, na.ACTS[acts[0]], acts[0])
                sys.stdout.flush()
            eng.set_encoder_reference(False)
    print("lane_faults %d" % eng.lane_faults())
    sys.exit(0)

if args.config5:
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import netref64 as nr
    bits = nr.edge_patches32(24)
    t = torch.from_numpy(bits.view(np.int64)).to(eng.device)
    wd1, bd1 = nr.dense1_32()
    for fam in ("shipped", "biased", "sat_conv1"):
        ws = nr.encoder_family(fam)
        ref = nr.encoder32_layers(ws, wd1, bd1, bits)
        eng.set_encoder_weights(ws)
        eng.set_encoder32_dense(wd1, bd1)
        p1, p2, f3, pre, out = (x.cpu().numpy() for x in eng.encode32_layers(t))
        print("32^3 encoder, family %s, %d edge patches, dense_1 bias U(-0.5, 0.5), against float64" % (fam, len(bits)))
        h = np.tanh(pre.astype(np.float64) + bd1.astype(np.float64))
        for name, a, b in (("P1", p1, ref[0]), ("P2", p2, ref[1]), ("F3", f3, ref[2]), ("tanh(Dense(200))", h, ref[3]), ("descriptors", out, ref[4])):
            d = np.abs(a.astype(np.float64) - b)
            print("%-18s max abs %.3e   mean abs %.3e   element-wise rel (floor 0.1) %.3e" % (name, d.max(), d.mean(), (d / np.maximum(np.abs(b), 0.1)).max()))
        sys.stdout.flush()
    print("lane_faults %d" % eng.lane_faults())
    sys.exit(0)

if args.family:
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import netref64 as nr
    bits = np.ascontiguousarray(np.concatenate([nr.edge_patches(70), golden_bits[::6]]))
    t = torch.from_numpy(bits.view(np.int64)).to(eng.device)
    for fam in (nr.ENCODER_FAMILIES if "all" in args.family else args.family):
        ws = nr.encoder_family(fam)
        ref = nr.encoder_layers(ws, bits)
        eng.set_encoder_weights(ws)
        for reference in (False, True):
            eng.set_encoder_reference(reference)
            layers = eng.encode_layers(t)
            torch.cuda.synchronize()
            print("family %s, %d patches, stage 1 = %s, against float64" % (fam, len(bits), "k_enc_stage1 (f32)" if reference else "k_enc_stage1x"))
            report(layers, ws[7], ref)
            sys.stdout.flush()
    sys.exit(0)

if os.environ.get("CAELO_ENC_S1") == "f32":   # (read HERE, by the tool: the library has no environment switch for arithmetic)
    eng.set_encoder_reference(True)
_, enc_m = orc.load_models(os.path.join(REPO, "weights", "SphericalRingPCRespondLayer.h5"), os.path.join(REPO, "weights", "EncoderModel4VoxelPatch.h5"))
layers = eng.encode_layers(torch.from_numpy(golden_bits.view(np.int64)).to(eng.device))
torch.cuda.synchronize()
report(layers, enc_m.w[7], enc_m.predict_layers(golden_bits))
