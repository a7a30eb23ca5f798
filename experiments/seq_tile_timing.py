"""dcll_conv_lif_sequence_tiles (k_lif_seq_tile: a 2-D grid of workgroups per sample) against the per-step net.test loop — the only
path these workloads have without it — and against dcll_conv_lif_sequence_bands where its rule serves every layer, every arm from
this tree.

    python experiments/seq_tile_timing.py [--runs 5] [--workloads radio2_24x40 radio1_48 ...] [--T N] [--out FILE]

Workloads (cell indices in, arp 1, T = 128 unless --T is given): radio_ml_conv.yaml at netscale 2 on 128x128 at B = 64
(`radio2_128`), at netscale 2 on 24x40 at B = 64 and 512 (`radio2_24x40`), at netscale 1 on 100x100 at B = 64 (`radio1_100`) and at
netscale 1 on 48x48 at B = 64 (`radio1_48`: the band rule serves it, so (0, 0) is `b0`; (3, 3) fits plain layers only and is refused with
a refractory trace, (2, 6) and (4, 4) fit).  Arms: `step` (the per-step
loop, graph replay as it defaults), `t0` (tiles=(0, 0), the library's rule), `tAxB` (tiles=(A, B)) and `b0` (bands=0).  An arm the
network does not serve is reported as refused.  The driver starts `runs` rounds of fresh child processes per workload, the arms
alternating within a round, each child under its own `timeout`; the first child that fails ends the run.  A child warms its path up
with two whole sequences, times `reps` sequences with a host clock around work that ends in a device synchronise, and prints one
JSON line; a fused child also brackets every layer's forward_sequence_any call with device events: an UPPER BOUND of the kernel
time (it holds the weight permutation, the snapshot, the zero fill, the allocations and the host's launch gap too).
"faster" (DESIGN §8's form): the slowest run of an arm is faster than the fastest run of the arm it is compared with."""
import argparse
import json
import os
import subprocess
import sys
import time

RADIO = dict(spec="radio_ml_conv.yaml", T=128, arp=1.0, target=24, reps=1)
WORKLOADS = dict(radio2_128=dict(RADIO, im=(1, 128, 128), batches=[64], netscale=2.0, arms=["step", "t0", "t13x16", "t16x16"]),
                 radio2_24x40=dict(RADIO, im=(1, 24, 40), batches=[64, 512], netscale=2.0, arms=["step", "t0", "t2x6", "t3x5", "t4x8"]),
                 radio1_100=dict(RADIO, im=(1, 100, 100), batches=[64], netscale=1.0, arms=["step", "t0", "t5x10", "t10x10"]),
                 radio1_48=dict(RADIO, im=(1, 48, 48), batches=[64], netscale=1.0, arms=["step", "b0", "t3x3", "t2x6", "t4x4"]))
TAG = "SEQ_TILE_TIMING "


def _how(arm):
    """the keyword arguments of test_sequence_any / forward_sequence_any of a fused arm"""
    if arm == "b0":
        return dict(wide=True, bands=0)
    if arm == "t0":
        return dict(tiles=(0, 0))
    ty, tx = arm[1:].split("x")
    return dict(tiles=(int(ty), int(tx)))


def child(arm, name, T_arg=None):
    sys.path.insert(0, os.getcwd())
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    wl = WORKLOADS[name]
    T, im, reps = T_arg or wl["T"], wl["im"], wl["reps"]
    how = _how(arm) if arm != "step" else {}
    dev = torch.device("cuda", 0)
    convs = load_network_spec(os.path.join(os.getcwd(), "snn_modulation_classification_amd", "networks", wl["spec"]))
    args = Namespace(netscale=wl["netscale"], alpha=.92, alphas=.85, alpharp=.65, arp=wl["arp"], lc_ampl=.5, random_tau=True)
    out = dict(arm=arm, workload=name, T=T, reps=reps)
    for B in wl["batches"]:
        torch.manual_seed(1)
        np.random.seed(1)
        net = ConvNetwork(args, im, B, convs, wl["target"], act=torch.nn.Sigmoid(), loss=None, opt=None, opt_param={},
                          learning_rates=None, burnin=20)
        net.reset(True)
        net.eval()
        assert not net.sequence_supported()
        if arm != "step" and not net.sequence_any_supported(**how):
            out["B%d" % B] = dict(refused=True)
            continue
        labels = np.zeros((B, wl["target"]), np.float32)
        labels[np.arange(B), np.arange(B) % wl["target"]] = 1
        cells = torch.from_numpy(np.random.RandomState(3).randint(0, im[1] * im[2], size=(T, B)).astype(np.int32)).to(dev)
        x = ops.cells_to_planes(cells, im[1] * im[2]).reshape(T, B, 1, im[1], im[2])
        assert tuple(x.shape) == (T, B) + tuple(im), x.shape

        def sequence():
            net.reset()
            if arm == "step":
                for t in range(T):
                    net.test(x[t])
            else:
                net.test_sequence_any(x, **how)

        for _ in range(2):
            sequence()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            sequence()
        torch.cuda.synchronize()
        y = torch.from_numpy(labels)[None].expand(T, -1, -1)
        rec = dict(ms_per_sequence=1e3 * (time.perf_counter() - t0) / reps,
                   vote=[int(v) for v in np.asarray(net.dcll_slices[-1]._predictions(y)[0])][:8])
        if arm != "step":
            net.reset()
            cur = ops.pack_spike_planes(x.reshape(T, B, im[0], im[1] * im[2]))
            layers = []
            for i, s in enumerate(net.dcll_slices):
                L = s.dclllayer
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                d = L.i2h.make_desc(L.im_dims, L.pooling, L.target_size, L.output_layer)
                with ops.kernel_trace() as tr:
                    e0.record()
                    spk, pv, _ = L.forward_sequence_any(cur, T, B, **how)
                    e1.record()
                torch.cuda.synchronize()
                by, bx = ops.sequence_tiles_plan(d, B, how["tiles"]) if "tiles" in how else (ops.sequence_bands_plan(d, B, 0), [0, 0])
                layers.append(dict(kernel=tr.names[-1], c_in=L.in_channels, c_out=L.out_channels, ms=e0.elapsed_time(e1),
                                   plan=[len(by) - 1, len(bx) - 1]))
                cur = spk
            rec["layers"] = layers
        out["B%d" % B] = rec
    print(TAG + json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--workloads", nargs="+", default=sorted(WORKLOADS), choices=sorted(WORKLOADS))
    p.add_argument("--arms", nargs="+", default=None, help="a subset of the workload's arms")
    p.add_argument("--child-timeout", type=int, default=150, help="seconds per child process")
    p.add_argument("--out", default=None, help="also write the table to this file")
    p.add_argument("--T", type=int, default=None, help="timesteps per sequence instead of the workload's 128")
    p.add_argument("--child")
    p.add_argument("--workload", choices=sorted(WORKLOADS))
    a = p.parse_args()
    if a.child:
        return child(a.child, a.workload, a.T)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "DCLL_HIP_SO"}
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("experiments/seq_tile_timing.py on one MI355X: per-step net.test loop | test_sequence_any(bands=0) | test_sequence_any(tiles=(A, B))")
    say()
    for name in a.workloads:
        wl = WORKLOADS[name]
        arms = [m for m in wl["arms"] if a.arms is None or m in a.arms]
        rows = []
        for r in range(a.runs):
            for arm in arms:
                cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", arm,
                       "--workload", name] + (["--T", str(a.T)] if a.T else [])
                res = subprocess.run(cmd, cwd=here, env=env, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
                if res.returncode != 0 or not line:         # (a fault, an abort or the time limit: nothing more is started)
                    sys.exit("child %s of run %d failed (%d):\n%s" % (arm, r, res.returncode, res.stderr[-2000:]))
                rec = json.loads(line[0][len(TAG):])
                rows.append(rec)
                print("run %d %-12s %-6s " % (r, name, arm) + "  ".join(
                    "B=%d: %s" % (b, "refused" if rec["B%d" % b].get("refused") else "%.2f ms" % rec["B%d" % b]["ms_per_sequence"])
                    for b in wl["batches"]), flush=True)
        say("%s at netscale %g on %dx%d, T = %d, ms per sequence (%d sequences per run, %d alternating fresh processes per arm)"
            % (wl["spec"], wl["netscale"], wl["im"][1], wl["im"][2], a.T or wl["T"], wl["reps"], a.runs))
        for b in wl["batches"]:
            say("  B = %d" % b)
            key = "B%d" % b
            ms = {arm: [x[key]["ms_per_sequence"] for x in rows if x["arm"] == arm and not x[key].get("refused")] for arm in arms}
            votes = [x[key]["vote"] for x in rows if not x[key].get("refused")]
            for arm in arms:
                if not ms[arm]:
                    say("    %-6s refused (a tile beyond the LDS, or more tiles than pooled pixels in some layer)" % arm)
                    continue
                text = "    %-6s %.2f-%.2f   [%s]" % (arm, min(ms[arm]), max(ms[arm]), " ".join("%.2f" % v for v in ms[arm]))
                for other in ("step", "b0"):
                    if arm != other and arm != "step" and ms.get(other):
                        text += "   vs %s: %s" % (other, "faster, %.2fx" % (min(ms[other]) / max(ms[arm])) if max(ms[arm]) < min(ms[other])
                                                   else "NOT faster")
                say(text)
            say("    output-layer votes of the first 8 samples equal in all runs of all arms: %s" % all(v == votes[0] for v in votes))
            for arm in arms:
                recs = [x[key] for x in rows if x["arm"] == arm and "layers" in x[key]]
                if not recs:
                    continue
                for i in range(len(recs[0]["layers"])):
                    ls = [x["layers"][i] for x in recs]
                    l = ls[-1]
                    say("    %-6s layer %d %3d -> %2d  %2d x %2d tiles  %-24s %.3f-%.3f ms per call (upper bound of the kernel)"
                        % (arm, i, l["c_in"], l["c_out"], max(l["plan"][0], 1), max(l["plan"][1], 1), l["kernel"],
                           min(x["ms"] for x in ls), max(x["ms"] for x in ls)))
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
