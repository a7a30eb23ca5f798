"""The learning timestep of radio_ml_conv_ref.yaml on the (16,128) plane with ConvNetwork.w3_step_path + w3_first_wgrad on in BOTH
arms and ConvNetwork.w3_dv_path off (every layer's dv plane from the generic k_bwd_dv — what the parent commit runs, in the same
library) and on (k_bwd_dv_w3), at B = 64 and B = 512.  After experiments/w3f_wgrad_timing.py.

    python experiments/w3_dv_timing.py [--runs 5] [--steps 30] [--batches 64 512] [--kernel_stats] [--out FILE]

The driver starts `runs` pairs of fresh child processes per batch size, one after another, alternating off / on, each under its own
time limit; the first child that fails ends the run.  A child (at most 16 CPU threads) builds the network, runs the burn-in and
warm-up steps (a small batch then replays its captured graph, as it defaults), times `steps` net.learn steps with a host clock
around work that ends in a device synchronise, and then brackets the open backward call of EVERY layer
(ops.conv_lif_backward(open_reduce=True): the dv kernel + the weight-gradient kernel, on the layer's own plane and inputs of the
layer's shapes) with device events around 20 calls.
--kernel_stats: one more child per arm and batch under `rocprofv3 --kernel-trace --stats` (a run of its own, the program behind
`--`: nothing else is traced, its times are not mixed with the others) that skips the learning steps and makes the 24 open backward
calls of one layer after another (1 logged + 3 warm-up + the 20 timed ones, the same inputs each time); the dv kernel's mean device
time per layer is taken from the kernel trace in launch order (24 dispatches per layer), and for k_bwd_dv_w3 its achieved
bytes/s — the bytes it has to move, B 64 h w 8 (v read, dv written; the product's call passes neither g_pv nor g_v) — against the
6.29 TB/s a float4 copy reaches on this part.
A library built with another DW_PER_BLOCK (experiments/build_variant.sh) is measured by DCLL_HIP_SO=<path>, which the children
inherit.
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
N_LAYERS = 7
BURNIN, WARM = 4, 10
COPY_TBS = 6.29
TAG = "W3_DV_TIMING "
CALLS = 24              # open backward calls of a layer in a child: 1 logged + 3 warm-up + 20 timed


def plane(i):
    """(h, w) of layer i's input = its un-pooled output plane: the width halves with every (1,2) pooling"""
    return HW[0], HW[1] >> i


def dv_bytes(B, i):
    h, w = plane(i)
    return B * 64 * h * w * 8


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
    net.w3_first_wgrad = True
    net.w3_dv_path = on
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
    rec["bwd_us"], rec["bwd_kernels"] = [], []
    x = xs[0]
    for li, s in enumerate(net.dcll_slices):
        L = s.dclllayer
        i = L.i2h
        desc = i.make_desc(x.shape[2:4], L.pooling, L.i2o.weight.shape[0], False)
        st = i.state
        sp, _, _, pv, v = ops.conv_lif_step(desc, x, i.weight, i.bias, i.alpha, i.tau_m__dt, i.alphas, i.tau_s__dt, st.eps0, st.eps1,
                                            st.arp, want_v=True, out={}, w3_path=True)
        g_p = torch.randn(B, 24, device=dev)
        gb = {}
        back = lambda: ops.conv_lif_backward(desc, st.eps1, v, pv, g_p, None, None, None, L.i2o.weight, want_out=False, out=gb,
                                             open_reduce=True, w3_path=True, w3_first=True, w3_dv=on)
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
        rec["bwd_us"].append(1e3 * e0.elapsed_time(e1) / 20)
        rec["bwd_kernels"].append(list(tr.names))
        x = sp
    print(TAG + json.dumps(rec), flush=True)


def kernel_stats(B, on, say):
    """mean device time (us) of the dv kernel per layer over the 24 open backward calls a --only_backward child makes of each layer,
    from rocprofv3's kernel trace: the seven layers launch the same kernel, so the dispatches are taken in launch order, CALLS per
    layer"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "w3dv", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(B), "--on", str(on), "--only_backward", "1"]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("profiled child B=%d on=%d failed (%d):\n%s" % (B, on, res.returncode, res.stderr[-2000:]))
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            say("  (no kernel trace file from rocprofv3: kernel times not reported)")
            return []
        rows = []
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "k_bwd_dv" in name and "nopool" not in name:
                    rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        rows.sort()
        if len(rows) != CALLS * N_LAYERS:
            say("  (%d dv dispatches in the trace, %d expected: kernel times not reported)" % (len(rows), CALLS * N_LAYERS))
            return []
        per = [[us for _, us in rows[CALLS * i:CALLS * (i + 1)]] for i in range(N_LAYERS)]
        return [(sum(t) / len(t), len(t)) for t in per]


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
    if os.environ.get("DCLL_HIP_SO"):
        say("library: %s" % os.environ["DCLL_HIP_SO"])
    for B in a.batches:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--child", str(B), "--on", str(on),
                       "--steps", str(a.steps)]
                res = subprocess.run(cmd, capture_output=True, text=True)
                print("B=%d run %d w3_dv_path %d: child done (%d)" % (B, r, on, res.returncode), file=sys.stderr, flush=True)
                line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
                if res.returncode != 0 or not line:         # (nothing more is started on the device behind a failed child)
                    sys.exit("child B=%d on=%d of run %d failed (%d):\n%s" % (B, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len(TAG):]))
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        say("radio_ml_conv_ref.yaml %dx%d B = %d, w3_step_path + w3_first_wgrad on in both arms (%d steps per run, %d alternating fresh "
            "processes each)" % (HW[0], HW[1], B, a.steps, a.runs))
        series = [("net.learn, ms per timestep", lambda x: x["learn_ms"], "%.3f")]
        series += [("layer %d (%dx%d) open backward call, us" % ((i,) + plane(i)), (lambda x, i=i: x["bwd_us"][i]), "%.1f")
                   for i in range(N_LAYERS)]
        for what, get, fmt in series:
            o, n = [get(x) for x in off], [get(x) for x in on]
            say("  %s" % what)
            say("    w3_dv_path off  " + " ".join(fmt % v for v in o) + ("   range " + fmt + " .. " + fmt) % (min(o), max(o)))
            say("    w3_dv_path on   " + " ".join(fmt % v for v in n) + ("   range " + fmt + " .. " + fmt) % (min(n), max(n)))
            say("    " + verdict(o, n))
        say("  kernels of layer 0 off: %s;  on: %s" % (", ".join(off[0]["bwd_kernels"][0]), ", ".join(on[0]["bwd_kernels"][0])))
        if a.kernel_stats:
            stats = {arm: kernel_stats(B, arm, say) for arm in (0, 1)}
            for i in range(N_LAYERS):
                for arm in (0, 1):
                    if i >= len(stats[arm]):
                        continue
                    us, calls = stats[arm][i]
                    extra = ""
                    if arm:
                        nbytes = dv_bytes(B, i)
                        extra = "   %.1f MB moved: %.2f TB/s = %.2f of the %.2f TB/s copy rate (traffic alone: %.1f us)" \
                            % (nbytes / 1e6, nbytes / us / 1e6, nbytes / us / 1e6 / COPY_TBS, COPY_TBS, nbytes / COPY_TBS / 1e6)
                    say("  dv kernel time, layer %d, w3_dv_path %s: %-12s %8.1f us mean of %d calls%s"
                        % (i, "on " if arm else "off", "k_bwd_dv_w3" if arm else "k_bwd_dv", us, calls, extra))
        say()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
# python experiments/w3_dv_timing.py --kernel_stats --out profiles/r15_w3_dv_timing.txt   (MI355X; the two batch sizes in two invocations: --batches 64, --batches 512)
