"""Networks a --netscale of 2 makes (layers of 33-64 output channels): the per-step net.test loop — the only path they had — against
ConvNetwork.test_sequence_any(wide=True) (k_lif_seq_wide), both from this tree.

    python experiments/seq_wide_timing.py [--runs 5] [--reps 2] [--workloads radio mnist] [--out FILE]

Workloads: radio_ml_conv.yaml at netscale 2 on the 16x16 plane (1 -> 64, 64 -> 64, 64 -> 64; arp 1), T = 128, cell indices in, at
B = 64 and B = 512; mnist_conv.yaml at netscale 2 (32 / 48 / 64 channels; arp 0), T = 50, image2spiketrain(gain=100), at B = 32
and B = 512.  The driver starts `runs` pairs of fresh child processes per workload, alternating the arms, each child under its own
`timeout`; the first child that fails ends the run.  A child warms its path up with two whole sequences (the per-step loop then
replays its captured graph, as it defaults), times `reps` sequences with a host clock around work that ends in a device
synchronise, and prints one JSON line.  The fused child also brackets every layer's forward_sequence_any call with device events:
an UPPER BOUND of the kernel time (it holds the weight permutation, the allocations and the host's launch gap too).  For layers on
k_lif_seq_wide that bound is reported as a share of the fp32-MFMA peak in algorithmic FLOPs and as the L2 read rate of the
streamed weights it implies (every wave reads the permuted matrix behind the part kept in LDS: 512 B per chain step), total and
per busy CU — DESIGN 4.1e compares it with the 66-73 GB/s per CU that rows shared by every workgroup reach.
"faster" (DESIGN §8's form): the slowest fused run is faster than the fastest per-step run."""
import argparse
import json
import os
import subprocess
import sys
import time

PEAK = 157.3e12         # fp32-input MFMA, FLOP/s (MI355X)
NCU = 256
WORKLOADS = dict(radio=dict(spec="radio_ml_conv.yaml", im=(1, 16, 16), T=128, batches=[64, 512], arp=1.0, target=24),
                 mnist=dict(spec="mnist_conv.yaml", im=(1, 28, 28), T=50, batches=[32, 512], arp=0.0, target=10))
LDS_MAX = 160 * 1024


def streamed_steps(L, B):
    """chain steps of a k_lif_seq_wide layer whose weights are read from L2 (csrc/dcll_seq_wide.hip: the launcher's nwl)"""
    from snn_modulation_classification_amd import ops
    i = L.i2h
    d = i.make_desc(L.im_dims, L.pooling, L.target_size, L.output_layer)
    base = ops.sequence_wide_lds(d) // 4
    kk = d.kh * d.kw
    steps = (d.c_in // 2) * kk + ((kk + 1) // 2 if d.c_in % 2 else 0)
    whole = (base + steps * 128) * 4 <= LDS_MAX
    budget = LDS_MAX // 2 if (not whole and B > 256 and base * 8 <= LDS_MAX) else LDS_MAX
    return steps - min(steps, (budget // 4 - base) // 128), steps


def child(mode, name, reps):
    sys.path.insert(0, os.getcwd())
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    wl = WORKLOADS[name]
    T, im = wl["T"], wl["im"]
    dev = torch.device("cuda", 0)
    convs = load_network_spec(os.path.join(os.getcwd(), "snn_modulation_classification_amd", "networks", wl["spec"]))
    args = Namespace(netscale=2.0, alpha=.92, alphas=.85, alpharp=.65, arp=wl["arp"], lc_ampl=.5, random_tau=True)
    out = dict(mode=mode, workload=name, T=T, reps=reps)
    for B in wl["batches"]:
        torch.manual_seed(1)
        np.random.seed(1)
        net = ConvNetwork(args, im, B, convs, wl["target"], act=torch.nn.Sigmoid(), loss=None, opt=None, opt_param={},
                          learning_rates=None, burnin=20)
        net.reset(True)
        net.eval()
        assert not net.sequence_supported() and net.sequence_any_supported(wide=True)
        labels = np.zeros((B, wl["target"]), np.float32)
        labels[np.arange(B), np.arange(B) % wl["target"]] = 1
        if name == "radio":
            from snn_modulation_classification_amd import ops
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
            if mode == "wide":
                net.test_sequence_any(x, wide=True)
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
        y = torch.from_numpy(labels)[None].expand(T, -1, -1)
        rec = dict(ms_per_sequence=1e3 * (time.perf_counter() - t0) / reps,
                   vote=[int(v) for v in np.asarray(net.dcll_slices[-1]._predictions(y)[0])][:8])
        if mode == "wide":
            from snn_modulation_classification_amd import ops
            net.reset()
            cur = ops.pack_spike_planes(x.reshape(T, B, im[0], im[1] * im[2]))
            layers = []
            for i, s in enumerate(net.dcll_slices):
                L = s.dclllayer
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with ops.kernel_trace() as tr:
                    e0.record()
                    spk, pv, _ = L.forward_sequence_any(cur, T, B, wide=True)
                    e1.record()
                torch.cuda.synchronize()
                ch, cw = L.i2h.get_output_shape(L.im_dims)
                kh, kw = L.i2h.kernel_size
                flop = 2.0 * T * B * L.out_channels * ch * cw * L.in_channels * kh * kw
                ms = e0.elapsed_time(e1)
                row = dict(kernel=tr.names[-1], c_in=L.in_channels, c_out=L.out_channels, ms=ms, gflop=flop / 1e9,
                           peak_frac=flop / (ms * 1e-3) / PEAK)
                if tr.names[-1].startswith("k_lif_seq_wide"):
                    streamed, steps = streamed_steps(L, B)
                    ntl = (ch * cw + 31) // 32
                    byts = 512.0 * streamed * ntl * T * B           # every pixel tile's chain reads the streamed steps once
                    row.update(streamed_steps=streamed, steps=steps, l2_gbs=byts / (ms * 1e-3) / 1e9,
                               l2_gbs_per_cu=byts / (ms * 1e-3) / 1e9 / min(B, NCU))
                layers.append(row)
                cur = spk
            rec["layers"] = layers
        out["B%d" % B] = rec
    print("SEQ_WIDE_TIMING " + json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--workloads", nargs="+", default=["radio", "mnist"], choices=sorted(WORKLOADS))
    p.add_argument("--child-timeout", type=int, default=150, help="seconds per child process")
    p.add_argument("--out", default=None, help="also write the table to this file")
    p.add_argument("--child", choices=["step", "wide"])
    p.add_argument("--workload", choices=sorted(WORKLOADS))
    a = p.parse_args()
    if a.child:
        return child(a.child, a.workload, a.reps)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "DCLL_HIP_SO"}
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("experiments/seq_wide_timing.py on one MI355X: per-step net.test loop (the only path these networks had) against "
        "ConvNetwork.test_sequence_any(wide=True)")
    say()
    for name in a.workloads:
        wl = WORKLOADS[name]
        rows = []
        for r in range(a.runs):
            for mode in ("step", "wide"):
                cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                       "--workload", name, "--reps", str(a.reps)]
                res = subprocess.run(cmd, cwd=here, env=env, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith("SEQ_WIDE_TIMING ")]
                if res.returncode != 0 or not line:         # (a fault, an abort or the time limit: nothing more is started)
                    sys.exit("child %s of run %d failed (%d):\n%s" % (mode, r, res.returncode, res.stderr[-2000:]))
                rec = json.loads(line[0][len("SEQ_WIDE_TIMING "):])
                rows.append(rec)
                print("run %d %-5s %-5s " % (r, name, mode) + "  ".join("B=%d: %.2f ms" % (b, rec["B%d" % b]["ms_per_sequence"])
                                                                       for b in wl["batches"]), flush=True)
        say("%s at netscale 2, T = %d, ms per sequence (%d sequences per run, %d alternating fresh processes per arm)"
            % (wl["spec"], wl["T"], a.reps, a.runs))
        for b in wl["batches"]:
            step = [x["B%d" % b]["ms_per_sequence"] for x in rows if x["mode"] == "step"]
            wide = [x["B%d" % b]["ms_per_sequence"] for x in rows if x["mode"] == "wide"]
            same = all(x["B%d" % b]["vote"] == rows[0]["B%d" % b]["vote"] for x in rows)
            say("  B = %d" % b)
            say("    per-step net.test loop (graph replay as it defaults): %.2f-%.2f   [%s]" % (min(step), max(step), " ".join("%.2f" % v for v in step)))
            say("    test_sequence_any(wide=True):                          %.2f-%.2f   [%s]" % (min(wide), max(wide), " ".join("%.2f" % v for v in wide)))
            say("    slowest fused %.2f %s fastest per-step %.2f -> %s; output-layer votes of the first 8 samples equal in all runs: %s"
                % (max(wide), "<" if max(wide) < min(step) else ">=", min(step),
                   "faster, %.2fx" % (min(step) / max(wide)) if max(wide) < min(step) else "NOT faster", same))
            for i in range(len(rows[1]["B%d" % b]["layers"])):
                ls = [x["B%d" % b]["layers"][i] for x in rows if x["mode"] == "wide"]
                l = ls[-1]
                text = "    layer %d %3d -> %2d %-22s %.3f-%.3f ms per call (upper bound of the kernel)  %.2f GFLOP  >= %.4f-%.4f of the fp32-MFMA peak" % (
                    i, l["c_in"], l["c_out"], l["kernel"], min(x["ms"] for x in ls), max(x["ms"] for x in ls), l["gflop"],
                    min(x["peak_frac"] for x in ls), max(x["peak_frac"] for x in ls))
                if l.get("streamed_steps"):
                    text += "; weights streamed from L2: %d of %d steps, %.0f-%.0f GB/s, %.1f-%.1f GB/s per busy CU" % (
                        l["streamed_steps"], l["steps"], min(x["l2_gbs"] for x in ls), max(x["l2_gbs"] for x in ls),
                        min(x["l2_gbs_per_cu"] for x in ls), max(x["l2_gbs_per_cu"] for x in ls))
                say(text)
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
