"""The learning timestep of radio_ml_conv_ref.yaml on the (16,128) plane with ConvNetwork.w3_step_path on in BOTH arms and
ConvNetwork.w3_first_wgrad off (the first layer's weight gradient on the generic k_bwd_wgrad — what the parent commit runs, in the
same library) and on (k_bwd_wgrad_w3f), at B = 64 and B = 512.  After experiments/w3_learn_timing.py.

    python experiments/w3f_wgrad_timing.py [--runs 5] [--steps 30] [--batches 64 512] [--kernel_stats] [--out FILE]

The driver starts `runs` pairs of fresh child processes per batch size, alternating off / on, each under its own time limit; the
first child that fails ends the run.  A child (at most 16 CPU threads) builds the network, runs the burn-in and warm-up steps (a
small batch then replays its captured graph, as it defaults), times `steps` net.learn steps with a host clock around work that ends
in a device synchronise, and then brackets layer 0's open backward call (ops.conv_lif_backward(open_reduce=True): k_bwd_dv + the
weight-gradient kernel) with device events around 20 calls.
--kernel_stats: one more child per arm and batch under `rocprofv3 --kernel-trace --stats` (a run of its own: nothing else is
traced, its times are not mixed with the others) that skips the learning steps and makes 24 open backward calls of layer 0 (1 logged + 3 warm-up + the 20 timed ones; the same
inputs each time, so all 24 do the same work and all are in rocprofv3's mean); the table then gives the mean
device time of k_bwd_dv and of the weight-gradient kernel, and for k_bwd_wgrad_w3f its achieved bytes/s — the bytes it has to read,
B 64 h w 4 (the dv plane) + B h w 4 (eps1) — against the 6.29 TB/s a float4 copy reaches on this part.
Ranges are printed, not means.  "faster" is said only where the slower end of the new range beats the faster end of the old one;
the margin is given relative to the larger of the two spreads."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

HW = (16, 128)
BATCHES = (64, 512)
BURNIN, WARM = 4, 10
COPY_TBS = 6.29
TAG = "W3F_WGRAD_TIMING "


def wgrad_bytes(B):
    return B * 64 * HW[0] * HW[1] * 4 + B * HW[0] * HW[1] * 4


def child(B, on, steps, only_backward):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from argparse import Namespace
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(5)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + HW) < .05).astype(np.float32)).to(dev) for _ in range(4)]
    y = torch.zeros(B, 24)
    y[np.arange(B), rng.randint(0, 24, size=B)] = 1
    y = y.to(dev)
    convs = load_network_spec(os.path.join(here, "snn_modulation_classification_amd", "networks", "radio_ml_conv_ref.yaml"))
    args = Namespace(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(args, (1,) + HW, B, convs, 24, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam,
                      opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6], burnin=BURNIN)
    net.reset(True)
    net.w3_step_path = True
    net.w3_first_wgrad = on
    net.train()
    rec = dict(B=B, on=on)
    if not only_backward:
        for t in range(BURNIN + WARM):
            net.learn(xs[t % 4], y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            net.learn(xs[t % 4], y)
        torch.cuda.synchronize()
        rec["learn_ms"] = 1e3 * (time.perf_counter() - t0) / steps
    L = net.dcll_slices[0].dclllayer
    i = L.i2h
    desc = i.make_desc(L.im_dims, L.pooling, L.i2o.weight.shape[0], False)
    st = i.state
    _, _, _, pv, v = ops.conv_lif_step(desc, xs[0], i.weight, i.bias, i.alpha, i.tau_m__dt, i.alphas, i.tau_s__dt, st.eps0, st.eps1,
                                       st.arp, want_v=True, out={}, w3_path=True)
    g_p = torch.randn(B, 24, device=dev)
    gb = {}
    back = lambda: ops.conv_lif_backward(desc, st.eps1, v, pv, g_p, None, None, None, L.i2o.weight, want_out=False, out=gb,
                                         open_reduce=True, w3_path=True, w3_first=on)
    with ops.kernel_trace() as tr:
        back()
    for _ in range(3):
        back()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        back()
    e1.record()
    torch.cuda.synchronize()
    rec.update(bwd_us=1e3 * e0.elapsed_time(e1) / 20, bwd_kernels=list(tr.names), nchunk=gb["parts"]["nchunk"])
    print(TAG + json.dumps(rec), flush=True)


def kernel_stats(B, on, say):
    """mean device time (us) per kernel over the 24 open backward calls of layer 0 that a --only_backward child makes (1 logged, 3
    warm-up, 20 timed: identical work), from rocprofv3's kernel statistics"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "200", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "w3f", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(B), "--on", str(on), "--only_backward", "1"]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("profiled child B=%d on=%d failed (%d):\n%s" % (B, on, res.returncode, res.stderr[-2000:]))
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            say("  (no kernel statistics file from rocprofv3: kernel times not reported)")
            return {}
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for key in ("k_bwd_wgrad_w3f", "k_bwd_wgrad", "k_bwd_dv"):
                    if key in name and key not in out and (key != "k_bwd_wgrad" or "k_bwd_wgrad_" not in name):
                        out[key] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
        return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--batches", type=int, nargs="+", default=list(BATCHES))
    p.add_argument("--kernel_stats", action="store_true")
    p.add_argument("--out")
    p.add_argument("--child", type=int)
    p.add_argument("--on", type=int, default=0)
    p.add_argument("--only_backward", type=int, default=0)
    a = p.parse_args()
    if a.child:
        return child(a.child, bool(a.on), a.steps, bool(a.only_backward))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def verdict(old, new):
        spread = max(max(old) - min(old), max(new) - min(new))
        if max(new) < min(old):
            return "faster: the slower end of the new range beats the faster end of the old one by %.1f x the larger spread (%.2fx .. %.2fx)" \
                % ((min(old) - max(new)) / max(spread, 1e-9), min(old) / max(new), max(old) / min(new))
        return "NOT faster: " + ("slower" if min(new) > max(old) else "the ranges overlap")
    for B in a.batches:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--child", str(B), "--on", str(on),
                       "--steps", str(a.steps)]
                res = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
                if res.returncode != 0 or not line:         # (nothing more is started on the device behind a failed child)
                    sys.exit("child B=%d on=%d of run %d failed (%d):\n%s" % (B, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len(TAG):]))
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        say("radio_ml_conv_ref.yaml %dx%d B = %d, w3_step_path on in both arms (%d steps per run, %d alternating fresh processes each)"
            % (HW[0], HW[1], B, a.steps, a.runs))
        for what, key, fmt in (("net.learn, ms per timestep", "learn_ms", "%.3f"), ("layer 0 open backward call, us", "bwd_us", "%.1f")):
            o, n = [x[key] for x in off], [x[key] for x in on]
            say("  %s" % what)
            say("    w3_first_wgrad off  " + " ".join(fmt % v for v in o) + ("   range " + fmt + " .. " + fmt) % (min(o), max(o)))
            say("    w3_first_wgrad on   " + " ".join(fmt % v for v in n) + ("   range " + fmt + " .. " + fmt) % (min(n), max(n)))
            say("    " + verdict(o, n))
        say("  kernels off: %s;  on: %s (%d partial rows)" % (", ".join(off[0]["bwd_kernels"]), ", ".join(on[0]["bwd_kernels"]), on[0]["nchunk"]))
        if a.kernel_stats:
            nbytes = wgrad_bytes(B)
            for arm in (0, 1):
                ks = kernel_stats(B, arm, say)
                for key, (us, calls) in sorted(ks.items()):
                    extra = ""
                    if key == "k_bwd_wgrad_w3f":
                        extra = "   %.1f MB read: %.2f TB/s = %.2f of the %.2f TB/s copy rate (traffic alone: %.1f us)" \
                            % (nbytes / 1e6, nbytes / us / 1e6, nbytes / us / 1e6 / COPY_TBS, COPY_TBS, nbytes / COPY_TBS / 1e6)
                    say("  kernel time, w3_first_wgrad %s: %-16s %8.1f us mean of %d calls%s" % ("on " if arm else "off", key, us, calls, extra))
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
# python experiments/w3f_wgrad_timing.py --kernel_stats --out profiles/r14_w3f_wgrad_timing.txt   (MI355X; the two batch sizes in two invocations: --batches 64, --batches 512)
