"""BASELINE config 1 (mnist_conv.yaml, 28x28, arp 0, T = 50, synthetic images through image2spiketrain(gain=100)): the per-step
net.test loop of the PARENT commit against this commit's ConvNetwork.test_sequence_any (k_lif_seq_any), at B = 32 and B = 512.

    python experiments/seq_any_timing.py --parent-tree DIR [--runs 5] [--reps 4]

DIR = a checkout of the parent commit with its libdcll_hip.so built (the parent's library is ABI 7: it is loaded by the parent's
own binding, DCLL_HIP_SO naming it, in a process whose import path is DIR).  The driver starts `runs` pairs of fresh child
processes, alternating parent / this commit; a child warms its path up with two whole sequences (the per-step loop then replays
its captured graph, as it defaults), times `reps` sequences with a host clock around work that ends in a device synchronise,
and prints one JSON line.  The fused child also brackets every layer's forward_sequence_any call with device events: an UPPER BOUND of the kernel time
(it holds k_seq_any_wprep, the allocations and the host's launch gap too; kernel durations: seq_any_kernel_times.py on a
rocprofv3 kernel trace of this child) and the share of the fp32-MFMA peak that bound implies for the algorithmic FLOPs.
The claim to check (DESIGN §8's form): the slowest fused run is faster than the fastest parent run, at both batches."""
import argparse
import json
import os
import subprocess
import sys
import time

T = 50
PEAK = 157.3e12         # fp32-input MFMA, FLOP/s (MI355X)


def child(mode, batches, reps):
    sys.path.insert(0, os.getcwd())
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    from snn_modulation_classification_amd.data.utils import image2spiketrain
    dev = torch.device("cuda", 0)
    convs = load_network_spec(os.path.join(os.getcwd(), "snn_modulation_classification_amd", "networks", "mnist_conv.yaml"))
    args = Namespace(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=0.0, lc_ampl=.5, random_tau=True)
    out = dict(mode=mode, T=T, reps=reps)
    for B in batches:
        torch.manual_seed(1)
        np.random.seed(1)
        net = ConvNetwork(args, (1, 28, 28), B, convs, 10, act=torch.nn.Sigmoid(), loss=None, opt=None, opt_param={},
                          learning_rates=None, burnin=20)
        net.reset(True)
        net.eval()
        g = torch.Generator().manual_seed(7)
        images = torch.rand(B, 28, 28, generator=g).numpy()
        labels = np.zeros((B, 10), np.float32)
        labels[np.arange(B), np.arange(B) % 10] = 1
        np.random.seed(3)
        sp, _ = image2spiketrain(images, labels, input_shape=(1, 28, 28), gain=100, min_duration=T - 1, max_duration=T)
        x = torch.Tensor(sp).to(dev)
        assert tuple(x.shape) == (T, B, 1, 28, 28), x.shape

        def sequence():
            net.reset()
            if mode == "any":
                net.test_sequence_any(x)
            else:
                for t in range(T):
                    net.test(x[t])

        for _ in range(2):
            sequence()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            sequence()
        torch.cuda.synchronize()
        rec = dict(ms_per_sequence=1e3 * (time.perf_counter() - t0) / reps,
                   vote=[int(v) for v in np.asarray(net.dcll_slices[-1]._predictions(torch.from_numpy(labels)[None].expand(T, -1, -1))[0])][:8])
        if mode == "any":
            from snn_modulation_classification_amd import ops
            net.reset()
            cur = ops.pack_spike_planes(x.reshape(T, B, 1, 28 * 28))
            layers = []
            for i, s in enumerate(net.dcll_slices):
                L = s.dclllayer
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with ops.kernel_trace() as tr:
                    e0.record()
                    spk, pv, _ = L.forward_sequence_any(cur, T, B)
                    e1.record()
                torch.cuda.synchronize()
                ch, cw = L.i2h.get_output_shape(L.im_dims)
                kh, kw = L.i2h.kernel_size
                flop = 2.0 * T * B * L.out_channels * ch * cw * L.in_channels * kh * kw
                ms = e0.elapsed_time(e1)
                layers.append(dict(kernel=tr.names[-1], ms=ms, gflop=flop / 1e9, peak_frac=flop / (ms * 1e-3) / PEAK))
                cur = spk
            rec["layers"] = layers
        out["B%d" % B] = rec
    print("SEQ_ANY_TIMING " + json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent-tree", required=False)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=4)
    p.add_argument("--batches", type=int, nargs="+", default=[32, 512])
    p.add_argument("--child", choices=["step", "any"])
    a = p.parse_args()
    if a.child:
        return child(a.child, a.batches, a.reps)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parent = os.path.abspath(a.parent_tree)
    plans = {"step": (parent, dict(os.environ, DCLL_HIP_SO=os.path.join(parent, "snn_modulation_classification_amd", "libdcll_hip.so"))),
             "any": (here, {k: v for k, v in os.environ.items() if k != "DCLL_HIP_SO"})}
    rows = []
    for r in range(a.runs):
        for mode in ("step", "any"):
            cwd, env = plans[mode]
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(a.reps), "--batches"] + [str(b) for b in a.batches]
            res = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=240)
            line = [l for l in res.stdout.splitlines() if l.startswith("SEQ_ANY_TIMING ")]
            if res.returncode != 0 or not line:
                sys.exit("child %s of run %d failed (%d):\n%s" % (mode, r, res.returncode, res.stderr[-2000:]))
            rec = json.loads(line[0][len("SEQ_ANY_TIMING "):])
            rows.append(rec)
            print("run %d %-4s " % (r, mode) + "  ".join("B=%d: %.2f ms" % (b, rec["B%d" % b]["ms_per_sequence"]) for b in a.batches), flush=True)
    print()
    for b in a.batches:
        step = [x["B%d" % b]["ms_per_sequence"] for x in rows if x["mode"] == "step"]
        any_ = [x["B%d" % b]["ms_per_sequence"] for x in rows if x["mode"] == "any"]
        same = all(x["B%d" % b]["vote"] == rows[0]["B%d" % b]["vote"] for x in rows)
        print("B = %d, T = %d, ms per sequence (%d sequences per run)" % (b, T, a.reps))
        print("  parent, per-step net.test loop (graph replay as it defaults): " + " ".join("%.2f" % v for v in step))
        print("  this commit, test_sequence_any:                               " + " ".join("%.2f" % v for v in any_))
        print("  slowest fused %.2f %s fastest parent %.2f -> %.2fx; output-layer votes of the first 8 samples equal in all runs: %s"
              % (max(any_), "<" if max(any_) < min(step) else ">=", min(step), min(step) / max(any_), same))
        last = [x for x in rows if x["mode"] == "any"][-1]["B%d" % b]["layers"]
        for i, l in enumerate(last):
            print("  layer %d  %-22s %.3f ms per call (upper bound of the kernel)  %.2f GFLOP  >= %.4f of the fp32-MFMA peak" % (i, l["kernel"], l["ms"], l["gflop"], l["peak_frac"]))
        print()


if __name__ == "__main__":
    main()
