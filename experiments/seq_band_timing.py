"""dcll_conv_lif_sequence_bands (k_lif_seq_band: several workgroups per sample) against the per-step net.test loop and against the
one-workgroup kernels (ConvNetwork.test_sequence_any(wide=True)), every arm from this tree.

    python experiments/seq_band_timing.py [--runs 5] [--workloads radio2 mnist1 mnist2 radio48] [--out FILE]

Workloads: radio_ml_conv.yaml at netscale 2 on the 16x16 plane (arp 1), T = 128, cell indices in, at B = 64 and 512;
mnist_conv.yaml at netscale 1 and 2 (arp 0), T = 50, image2spiketrain(gain=100), at B = 32 and 512; radio_ml_conv.yaml at netscale
1 on a 48x48 plane at B = 64, which no one-workgroup path serves (per-step loop against bands = 0 only).  Arms: `step` (the
per-step loop, graph replay as it defaults), `wide` (test_sequence_any(wide=True), bands=None), `b2` / `b4` / `b8` (bands = 2 / 4 /
8) and `b0` (the library's rule).  An arm whose band count the network does not serve (a band beyond the LDS, more bands than
pooled rows) is reported as refused.  The driver starts `runs` rounds of fresh child processes per workload, the arms alternating
within a round, each child under its own `timeout`; the first child that fails ends the run.  A child warms its path up with two
whole sequences, times `reps` sequences with a host clock around work that ends in a device synchronise, and prints one JSON line;
a fused child also brackets every layer's forward_sequence_any call with device events: an UPPER BOUND of the kernel time (it holds
the weight permutation, the snapshot, the allocations and the host's launch gap too).
"faster" (DESIGN §8's form): the slowest run of an arm is faster than the fastest run of the arm it is compared with."""
import argparse
import json
import os
import subprocess
import sys
import time

WORKLOADS = dict(radio2=dict(spec="radio_ml_conv.yaml", im=(1, 16, 16), T=128, batches=[64, 512], arp=1.0, target=24, netscale=2.0,
                             arms=["step", "wide", "b2", "b4", "b8", "b0"], reps=2),
                 mnist1=dict(spec="mnist_conv.yaml", im=(1, 28, 28), T=50, batches=[32, 512], arp=0.0, target=10, netscale=1.0,
                             arms=["step", "wide", "b2", "b4", "b8", "b0"], reps=2),
                 mnist2=dict(spec="mnist_conv.yaml", im=(1, 28, 28), T=50, batches=[32, 512], arp=0.0, target=10, netscale=2.0,
                             arms=["step", "wide", "b2", "b4", "b8", "b0"], reps=2),
                 radio48=dict(spec="radio_ml_conv.yaml", im=(1, 48, 48), T=128, batches=[64], arp=1.0, target=24, netscale=1.0,
                              arms=["step", "b0"], reps=1))
TAG = "SEQ_BAND_TIMING "


def child(arm, name):
    sys.path.insert(0, os.getcwd())
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    wl = WORKLOADS[name]
    T, im, reps = wl["T"], wl["im"], wl["reps"]
    bands = int(arm[1:]) if arm[0] == "b" else None
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
        if arm != "step" and not net.sequence_any_supported(wide=True, bands=bands):
            out["B%d" % B] = dict(refused=True)
            continue
        labels = np.zeros((B, wl["target"]), np.float32)
        labels[np.arange(B), np.arange(B) % wl["target"]] = 1
        if name.startswith("radio"):
            cells = torch.from_numpy(np.random.RandomState(3).randint(0, im[1] * im[2], size=(T, B)).astype(np.int32)).to(dev)
            x = ops.cells_to_planes(cells, im[1] * im[2]).reshape(T, B, 1, im[1], im[2])
        else:
            from snn_modulation_classification_amd.data.utils import image2spiketrain
            g = torch.Generator().manual_seed(7)
            images = torch.rand(B, 28, 28, generator=g).numpy()
            np.random.seed(3)
            sp, _ = image2spiketrain(images, labels, input_shape=im, gain=100, min_duration=T - 1, max_duration=T)
            x = torch.Tensor(sp).to(dev)
        assert tuple(x.shape) == (T, B) + tuple(im), x.shape

        def sequence():
            net.reset()
            if arm == "step":
                for t in range(T):
                    net.test(x[t])
            else:
                net.test_sequence_any(x, wide=True, bands=bands)

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
                    spk, pv, _ = L.forward_sequence_any(cur, T, B, wide=True, bands=bands)
                    e1.record()
                torch.cuda.synchronize()
                plan = ops.sequence_bands_plan(d, B, bands) if bands is not None else [0, 0]
                layers.append(dict(kernel=tr.names[-1], c_in=L.in_channels, c_out=L.out_channels, ms=e0.elapsed_time(e1),
                                   bands=len(plan) - 1))
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
    p.add_argument("--child")
    p.add_argument("--workload", choices=sorted(WORKLOADS))
    a = p.parse_args()
    if a.child:
        return child(a.child, a.workload)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "DCLL_HIP_SO"}
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("experiments/seq_band_timing.py on one MI355X: per-step net.test loop | test_sequence_any(wide=True) | test_sequence_any(bands=N)")
    say()
    for name in a.workloads:
        wl = WORKLOADS[name]
        arms = [m for m in wl["arms"] if a.arms is None or m in a.arms]
        rows = []
        for r in range(a.runs):
            for arm in arms:
                cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", arm,
                       "--workload", name]
                res = subprocess.run(cmd, cwd=here, env=env, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
                if res.returncode != 0 or not line:         # (a fault, an abort or the time limit: nothing more is started)
                    sys.exit("child %s of run %d failed (%d):\n%s" % (arm, r, res.returncode, res.stderr[-2000:]))
                rec = json.loads(line[0][len(TAG):])
                rows.append(rec)
                print("run %d %-7s %-5s " % (r, name, arm) + "  ".join(
                    "B=%d: %s" % (b, "refused" if rec["B%d" % b].get("refused") else "%.2f ms" % rec["B%d" % b]["ms_per_sequence"])
                    for b in wl["batches"]), flush=True)
        say("%s at netscale %g on %dx%d, T = %d, ms per sequence (%d sequences per run, %d alternating fresh processes per arm)"
            % (wl["spec"], wl["netscale"], wl["im"][1], wl["im"][2], wl["T"], wl["reps"], a.runs))
        for b in wl["batches"]:
            say("  B = %d" % b)
            key = "B%d" % b
            ms = {arm: [x[key]["ms_per_sequence"] for x in rows if x["arm"] == arm and not x[key].get("refused")] for arm in arms}
            votes = [x[key]["vote"] for x in rows if not x[key].get("refused")]
            for arm in arms:
                if not ms[arm]:
                    say("    %-5s refused (a band beyond the LDS, or more bands than pooled rows in some layer)" % arm)
                    continue
                text = "    %-5s %.2f-%.2f   [%s]" % (arm, min(ms[arm]), max(ms[arm]), " ".join("%.2f" % v for v in ms[arm]))
                for other in ("step", "wide"):
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
                    say("    %-5s layer %d %3d -> %2d  %d band(s)  %-24s %.3f-%.3f ms per call (upper bound of the kernel)"
                        % (arm, i, l["c_in"], l["c_out"], max(l["bands"], 1), l["kernel"], min(x["ms"] for x in ls), max(x["ms"] for x in ls)))
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
