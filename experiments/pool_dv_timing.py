"""The learning timestep with ConvNetwork.pool_dv_path off (the dv plane of the pooling layers from the generic k_bwd_dv — the same
tree with the flag off) and on (k_bwd_dv_pool), in ms, on mnist_conv.yaml (pooling 2 / 1 / 2, 28x28, arp 0, T = 50):

    mnist-ns1-B32, mnist-ns1-B512    netscale 1 (16 / 24 / 32 channels), any_learning_path + any_step_path in both arms
    mnist-ns2-B32, mnist-ns2-B512    netscale 2 (32 / 48 / 64 channels), wide_learning_path + wide_step_path in both arms

    python experiments/pool_dv_timing.py [--runs 5] [--workloads ...] [--kernel_stats] [--out FILE]

The driver starts `runs` pairs of fresh child processes per workload, alternating off / on.  A child builds the network, runs the
burn-in and 12 warm-up learning steps (the small batch then replays its captured graph, as it defaults), times T learning steps with a
host clock around work that ends in a device synchronise, and then brackets each slice's open backward call (dv + weight gradient, no
output_ gradient) with device events, 20 calls each.  --kernel_stats: one more child per arm of mnist-ns2-B512 under `rocprofv3
--kernel-trace --stats` (a run of its own, the program behind `--`; only the per-layer calls: 24 of each layer) for the two dv
kernels' own times, with the kernel's compulsory bytes (v read, dv written, i2o_W and g_p read once) against the 6.29 TB/s copy rate.
Ranges are printed, not means; "faster" is said only where the slow end of the new range beats the fast end of the old one."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

WORKLOADS = {"mnist-ns1-B32": (1.0, 32), "mnist-ns1-B512": (1.0, 512), "mnist-ns2-B32": (2.0, 32), "mnist-ns2-B512": (2.0, 512)}
SPEC, HW, TARGET, STEPS = "mnist_conv.yaml", (28, 28), 10, 50
BURNIN, WARM, CALLS = 4, 12, 24
COPY_RATE = 6.29e12         # bytes / s: the copy rate this project measures against (experiments/fill_bw.py)
TAG = "POOL_DV_TIMING "


def child(workload, on, only_backward):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    netscale, B = WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    convs = load_network_spec(os.path.join(here, "snn_modulation_classification_amd", "networks", SPEC))
    args = Namespace(netscale=netscale, alpha=.92, alphas=.85, alpharp=.65, arp=0.0, lc_ampl=.5, random_tau=True)
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(args, (1,) + HW, B, convs, TARGET, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam,
                      opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6], burnin=BURNIN)
    net.reset(True)
    net.train()
    wide = netscale > 1
    if wide:
        net.wide_learning_path = net.wide_step_path = True
    else:
        net.any_learning_path = net.any_step_path = True
    net.pool_dv_path = on
    rng = np.random.RandomState(5)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + HW) < .1).astype(np.float32)).to(dev) for _ in range(8)]
    y = torch.zeros(B, TARGET)
    y[np.arange(B), rng.randint(0, TARGET, size=B)] = 1
    y = y.to(dev)
    rec = dict(workload=workload, on=on, ms_per_step=None, layers=[])
    for t in range(BURNIN + (0 if only_backward else WARM)):
        net.learn(xs[t % 8], y)
    torch.cuda.synchronize()
    if not only_backward:
        t0 = time.perf_counter()
        for t in range(STEPS):
            net.learn(xs[t % 8], y)
        torch.cuda.synchronize()
        rec["ms_per_step"] = 1e3 * (time.perf_counter() - t0) / STEPS
    for s in net.dcll_slices:
        L = s.dclllayer
        desc = L.i2h.make_desc(L.im_dims, L.pooling, L.i2o.weight.shape[0], L.output_layer)
        ch, cw, ph, pw = ops.conv_out_shape(desc)
        v = torch.randn(B, L.out_channels, ch, cw, device=dev)
        g_p = torch.randn(B, L.i2o.weight.shape[0], device=dev)
        out = {}
        call = lambda: ops.conv_lif_backward(desc, L.i2h.state.eps1, v, None, g_p, None, None, None, L.i2o.weight, want_out=False, out=out,
                                             open_reduce=True, wide_path=wide, any_path=not wide, pool_dv=on)
        with ops.kernel_trace() as tr:
            call()
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS - 4):
            call()
        e1.record()
        torch.cuda.synchronize()
        K = L.out_channels * ph * pw
        rec["layers"].append(dict(kernels=tr.names, us=1e3 * e0.elapsed_time(e1) / (CALLS - 4), pool=list(L.pooling),
                                  plane=[B, L.out_channels, ch, cw], K=K,
                                  bytes=4 * (2 * B * L.out_channels * ch * cw + TARGET * K + B * TARGET)))
    print(TAG + json.dumps(rec), flush=True)


def kernel_stats(workload, on, say):
    """mean device time (us) of the dv kernel of each pooling layer over the CALLS open backward calls an --only_backward child makes
    of each layer, from rocprofv3's kernel trace (dispatches in launch order, CALLS per layer) -> [(mean us, calls, bytes)]"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "pooldv", "--",
               sys.executable, os.path.abspath(__file__), "--child", workload, "--on", str(on), "--only_backward", "1"]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("profiled child %s on=%d failed (%d):\n%s" % (workload, on, res.returncode, res.stderr[-2000:]))
        line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
        layers = [l for l in json.loads(line[0][len(TAG):])["layers"] if l["pool"] != [1, 1]] if line else []
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files or not layers:
            say("  (no kernel trace file from rocprofv3: kernel times not reported)")
            return []
        rows = []
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "k_bwd_dv" in name and "nopool" not in name:
                    rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        rows.sort()
        rows = rows[len(rows) - CALLS * len(layers):]           # (behind the learning steps of the burn-in, which launch none)
        if len(rows) != CALLS * len(layers):
            say("  (%d dv dispatches in the trace, %d expected: kernel times not reported)" % (len(rows), CALLS * len(layers)))
            return []
        per = [[us for _, us in rows[CALLS * i:CALLS * (i + 1)]] for i in range(len(layers))]
        return [(sum(t) / len(t), len(t), l) for t, l in zip(per, layers)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    p.add_argument("--kernel_stats", action="store_true")
    p.add_argument("--out")
    p.add_argument("--child")
    p.add_argument("--on", type=int, default=0)
    p.add_argument("--only_backward", type=int, default=0)
    a = p.parse_args()
    if a.child:
        return child(a.child, bool(a.on), bool(a.only_backward))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def verdict(old, new):
        if max(new) < min(old):
            return "faster (%.2fx .. %.2fx)" % (min(old) / max(new), max(old) / min(new))
        return "NOT faster: " + ("slower" if min(new) > max(old) else "the ranges overlap")
    for wl in a.workloads:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", wl, "--on", str(on)]
                res = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
                if res.returncode != 0 or not line:         # (nothing more is started on the GPU behind a failed child)
                    sys.exit("child %s on=%d of run %d failed (%d):\n%s" % (wl, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len(TAG):]))
                print("  (%s run %d %s: %.3f ms)" % (wl, r, "on" if on else "off", rows[-1]["ms_per_step"]), flush=True)
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        ms = lambda rs: [x["ms_per_step"] for x in rs]
        say("%s: net.learn, ms per timestep (%d steps per run, %d alternating fresh processes each; %s in both arms)"
            % (wl, STEPS, a.runs, "wide_learning_path + wide_step_path" if WORKLOADS[wl][0] > 1 else "any_learning_path + any_step_path"))
        say("  flag off      " + " ".join("%.3f" % v for v in ms(off)) + "   range %.3f .. %.3f" % (min(ms(off)), max(ms(off))))
        say("  pool_dv_path  " + " ".join("%.3f" % v for v in ms(on)) + "   range %.3f .. %.3f" % (min(ms(on)), max(ms(on))))
        say("  pool_dv_path: " + verdict(ms(off), ms(on)))
        for i in range(len(off[0]["layers"])):
            us = {name: [x["layers"][i]["us"] for x in rs] for name, rs in (("off", off), ("on", on))}
            for name, rs in (("off", off), ("on", on)):
                dv = [k for k in rs[0]["layers"][i]["kernels"] if k.startswith("k_bwd_dv")]
                say("  layer %d (pool %s) %-3s open backward call (dv + weight gradient) %.1f .. %.1f us   %s"
                    % (i, "x".join(map(str, rs[0]["layers"][i]["pool"])), name, min(us[name]), max(us[name]), ", ".join(dv)))
            say("  layer %d: %s" % (i, verdict(us["off"], us["on"]) if off[0]["layers"][i]["pool"] != [1, 1] else "no pooling: the same call in both arms"))
        say()
    if a.kernel_stats:
        wl = "mnist-ns2-B512"
        say("%s: the dv kernels' own times (rocprofv3 --kernel-trace --stats, one run per arm, mean of %d calls per layer)" % (wl, CALLS))
        for on in (0, 1):
            for mean, n, l in kernel_stats(wl, on, say):
                floor = 1e6 * l["bytes"] / COPY_RATE
                say("  %-13s plane %s pool %s K %d: %.1f us (%d calls); %.1f MB per launch (v read, dv written, i2o_W and g_p once), "
                    "%.1f us at 6.29 TB/s: %.2f of the copy rate"
                    % ("k_bwd_dv_pool" if on else "k_bwd_dv", "x".join(map(str, l["plane"])), "x".join(map(str, l["pool"])), l["K"], mean, n,
                       l["bytes"] / 1e6, floor, floor / mean))
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
