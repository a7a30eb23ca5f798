"""The per-step timesteps with ConvNetwork.any_step_path off (dcll_conv_lif_step's dispatch — what the parent commit runs) and on
(k_lif_step_any), in ms, on four workloads:

    config1-B32, config1-B512    mnist_conv.yaml, 28x28, arp 0 (BASELINE config 1)
    radio24-B64, radio24-B512    radio_ml_conv.yaml on the 24x24 plane, arp 1 (B = 64: the split form, three workgroups per
                                 sample; B = 512: the fused form)
and three timesteps each: net.test(x[t]), net.learn(x[t], y), and net.learn with any_learning_path on BOTH sides.

    python experiments/step_any_timing.py [--runs 5] [--steps 40] [--out FILE]

The driver starts `runs` pairs of fresh child processes per workload, alternating off / on.  A child builds the network, runs the
burn-in and 12 warm-up steps of each kind (a small batch then replays its captured graph, as it defaults), times `steps` steps
with a host clock around work that ends in a device synchronise, and then brackets each layer's step call (ops.conv_lif_step
without readouts, state advancing) with device events, 20 calls each: the layer kernels plus the host's launch gaps — the same
bound for both paths.  Ranges are printed, not means; the bound for the new path is the default path's own time for the same
step."""
import argparse
import json
import os
import subprocess
import sys
import time

WORKLOADS = {"config1-B32": ("mnist_conv.yaml", (28, 28), 32, 10, 0.0), "config1-B512": ("mnist_conv.yaml", (28, 28), 512, 10, 0.0),
             "radio24-B64": ("radio_ml_conv.yaml", (24, 24), 64, 24, 1.0), "radio24-B512": ("radio_ml_conv.yaml", (24, 24), 512, 24, 1.0)}
BURNIN, WARM = 4, 12
KINDS = ("test", "learn", "learn+any_learning_path")


def child(workload, on, steps):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    spec, hw, B, target, arp = WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(5)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .1).astype(np.float32)).to(dev) for _ in range(8)]
    y = torch.zeros(B, target)
    y[np.arange(B), rng.randint(0, target, size=B)] = 1
    y = y.to(dev)
    rec = dict(workload=workload, on=on, ms={}, layers=[])
    net = None
    for kind in KINDS:
        convs = load_network_spec(os.path.join(here, "snn_modulation_classification_amd", "networks", spec))
        args = Namespace(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=arp, lc_ampl=.5, random_tau=True)
        torch.manual_seed(1)
        np.random.seed(1)
        net = ConvNetwork(args, (1,) + hw, B, convs, target, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam,
                          opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6], burnin=BURNIN)
        net.reset(True)
        net.any_step_path = on
        if kind == "test":
            step = lambda t: net.test(xs[t % 8])
        else:
            net.train()
            net.any_learning_path = kind != "learn"
            step = lambda t: net.learn(xs[t % 8], y)
        for t in range(BURNIN + WARM):
            step(t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            step(t)
        torch.cuda.synchronize()
        rec["ms"][kind] = 1e3 * (time.perf_counter() - t0) / steps
    cur = xs[0]
    for s in net.dcll_slices:
        L = s.dclllayer
        i = L.i2h
        desc = i.make_desc(L.im_dims, L.pooling, 0, False)
        st = i.state
        out = {}
        call = lambda: ops.conv_lif_step(desc, cur, i.weight, i.bias, i.alpha, i.tau_m__dt, i.alphas, i.tau_s__dt, st.eps0, st.eps1,
                                         st.arp if len(st) > 2 else None, want_v=False, out=out, any_path=on)
        with ops.kernel_trace() as tr:
            nxt = call()[0]
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call()
        e1.record()
        torch.cuda.synchronize()
        rec["layers"].append(dict(kernels=tr.names, us=1e3 * e0.elapsed_time(e1) / 20))
        cur = nxt.clone()
    print("STEP_ANY_TIMING " + json.dumps(rec))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    p.add_argument("--out")
    p.add_argument("--child")
    p.add_argument("--on", type=int, default=0)
    a = p.parse_args()
    if a.child:
        return child(a.child, bool(a.on), a.steps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    for wl in a.workloads:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", wl, "--on", str(on), "--steps", str(a.steps)]
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
                line = [l for l in res.stdout.splitlines() if l.startswith("STEP_ANY_TIMING ")]
                if res.returncode != 0 or not line:
                    sys.exit("child %s on=%d of run %d failed (%d):\n%s" % (wl, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len("STEP_ANY_TIMING "):]))
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        say("%s: timesteps, ms (%d steps per run, %d alternating fresh processes each)" % (wl, a.steps, a.runs))
        for kind in KINDS:
            ms = lambda rs: [x["ms"][kind] for x in rs]
            say("  net.%-24s default path  " % kind + " ".join("%.3f" % v for v in ms(off)) + "   range %.3f .. %.3f" % (min(ms(off)), max(ms(off))))
            say("  net.%-24s any_step_path " % kind + " ".join("%.3f" % v for v in ms(on)) + "   range %.3f .. %.3f" % (min(ms(on)), max(ms(on))))
            verdict = "faster" if max(ms(on)) < min(ms(off)) else "slower" if min(ms(on)) > max(ms(off)) else "ranges overlap"
            say("  any_step_path: %s" % verdict)
        for i in range(len(off[0]["layers"])):
            for name, rs in (("default", off), ("any", on)):
                us = [x["layers"][i]["us"] for x in rs]
                say("  layer %d %-8s step call %.1f .. %.1f us   %s" % (i, name, min(us), max(us), ", ".join(rs[0]["layers"][i]["kernels"])))
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
