"""The learning timestep with ConvNetwork.wide_learning_path off (the default weight-gradient dispatch: the generic VALU k_bwd_wgrad
for every layer above 32 output channels — the same tree with the flag off) and on (k_bwd_wgrad_wide; k_bwd_wgrad_any for a layer of
at most 32 channels), in ms, on the networks a --netscale of 2 makes:

    radio-ns2-B64, radio-ns2-B512    radio_ml_conv.yaml at netscale 2 on 16x16 (1 -> 64, 64 -> 64, 64 -> 64), arp 1, T = 128
    mnist-ns2-B32, mnist-ns2-B512    mnist_conv.yaml at netscale 2 (32 / 48 / 64 channels), 28x28, arp 0, T = 50

    python experiments/bwd_wide_timing.py [--runs 5] [--workloads ...] [--out FILE]

The driver starts `runs` pairs of fresh child processes per workload, alternating off / on.  A child builds the network, runs the
burn-in and 12 warm-up learning steps (the small batch then replays its captured graph, as it defaults), times T learning
steps with a host clock around work that ends in a device synchronise, and then brackets each slice's open backward call
(dv + weight gradient, no output_ gradient) with device events, 20 calls each: an UPPER BOUND of the weight-gradient kernel's time
that holds the dv kernel and the host's launch gap too — the same bound for both paths.  Ranges are printed, not means; "faster" is
said only where the slow end of the new range beats the fast end of the old one."""
import argparse
import json
import os
import subprocess
import sys
import time

WORKLOADS = {"radio-ns2-B64": ("radio_ml_conv.yaml", (16, 16), 64, 24, 1.0, 128), "radio-ns2-B512": ("radio_ml_conv.yaml", (16, 16), 512, 24, 1.0, 128),
             "mnist-ns2-B32": ("mnist_conv.yaml", (28, 28), 32, 10, 0.0, 50), "mnist-ns2-B512": ("mnist_conv.yaml", (28, 28), 512, 10, 0.0, 50)}
NETSCALE = 2.0
BURNIN, WARM = 4, 12


def child(workload, on):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    spec, hw, B, target, arp, steps = WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    convs = load_network_spec(os.path.join(here, "snn_modulation_classification_amd", "networks", spec))
    args = Namespace(netscale=NETSCALE, alpha=.92, alphas=.85, alpharp=.65, arp=arp, lc_ampl=.5, random_tau=True)
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(args, (1,) + hw, B, convs, target, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam,
                      opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6], burnin=BURNIN)
    net.reset(True)
    net.train()
    net.wide_learning_path = on
    rng = np.random.RandomState(5)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .1).astype(np.float32)).to(dev) for _ in range(8)]
    y = torch.zeros(B, target)
    y[np.arange(B), rng.randint(0, target, size=B)] = 1
    y = y.to(dev)
    for t in range(BURNIN + WARM):
        net.learn(xs[t % 8], y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        net.learn(xs[t % 8], y)
    torch.cuda.synchronize()
    rec = dict(workload=workload, on=on, ms_per_step=1e3 * (time.perf_counter() - t0) / steps, layers=[])
    for s in net.dcll_slices:
        L = s.dclllayer
        desc = L.i2h.make_desc(L.im_dims, L.pooling, L.i2o.weight.shape[0], L.output_layer)
        ch, cw, ph, pw = ops.conv_out_shape(desc)
        v = torch.randn(B, L.out_channels, ch, cw, device=dev)
        g_p = torch.randn(B, L.i2o.weight.shape[0], device=dev)
        out = {}
        call = lambda: ops.conv_lif_backward(desc, L.i2h.state.eps1, v, None, g_p, None, None, None, L.i2o.weight, want_out=False, out=out,
                                             open_reduce=True, wide_path=on)
        with ops.kernel_trace() as tr:
            call()
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call()
        e1.record()
        torch.cuda.synchronize()
        rec["layers"].append(dict(kernels=tr.names, us=1e3 * e0.elapsed_time(e1) / 20))
    print("BWD_WIDE_TIMING " + json.dumps(rec))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    p.add_argument("--out")
    p.add_argument("--child")
    p.add_argument("--on", type=int, default=0)
    a = p.parse_args()
    if a.child:
        return child(a.child, bool(a.on))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    for wl in a.workloads:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", wl, "--on", str(on)]
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
                line = [l for l in res.stdout.splitlines() if l.startswith("BWD_WIDE_TIMING ")]
                if res.returncode != 0 or not line:
                    sys.exit("child %s on=%d of run %d failed (%d):\n%s" % (wl, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len("BWD_WIDE_TIMING "):]))
                print("  (%s run %d %s: %.3f ms)" % (wl, r, "on" if on else "off", rows[-1]["ms_per_step"]), flush=True)
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        ms = lambda rs: [x["ms_per_step"] for x in rs]
        say("%s: learning timestep, ms (%d steps per run, %d alternating fresh processes each)" % (wl, WORKLOADS[wl][5], a.runs))
        say("  default path       " + " ".join("%.3f" % v for v in ms(off)) + "   range %.3f .. %.3f" % (min(ms(off)), max(ms(off))))
        say("  wide_learning_path " + " ".join("%.3f" % v for v in ms(on)) + "   range %.3f .. %.3f" % (min(ms(on)), max(ms(on))))
        verdict = "faster" if max(ms(on)) < min(ms(off)) else "slower" if min(ms(on)) > max(ms(off)) else "ranges overlap"
        say("  wide path: %s (%.2fx .. %.2fx)" % (verdict, min(ms(off)) / max(ms(on)), max(ms(off)) / min(ms(on))))
        for i in range(len(off[0]["layers"])):
            for name, rs in (("default", off), ("wide", on)):
                us = [x["layers"][i]["us"] for x in rs]
                wg = [k for k in rs[0]["layers"][i]["kernels"] if k.startswith("k_bwd_wgrad")]
                say("  layer %d %-8s open backward call (dv + weight gradient) %.1f .. %.1f us   %s" % (i, name, min(us), max(us), ", ".join(wg)))
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
