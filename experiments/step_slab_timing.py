"""The inference and learning timesteps with ConvNetwork.slab_step_path off (dcll_conv_lif_step's dispatch: k_trace + k_conv_lif_tiled +
k_pool on the vector pipe for every layer above 32 output channels — the same tree with the flag off) and on (k_lif_step_slab in
bands of rows x slabs of 64 output channels; dcll_conv_lif_step_wide's kernels for a layer that call serves), in ms, with
slab_learning_path on in BOTH arms, on the networks a --netscale of 3 or 4 makes and on a plane the 64-channel step kernel refuses:

    radio-ns3-B64, -B128, -B512      radio_ml_conv.yaml at netscale 3 on 16x16 (1 -> 96, 96 -> 96, 96 -> 96), arp 1, T = 128
    radio-ns4-B64, -B128, -B512      radio_ml_conv.yaml at netscale 4 on 16x16 (1 -> 128, 128 -> 128, 128 -> 128)
    radio-ns2-24x40-B64              radio_ml_conv.yaml at netscale 2 on 24x40 (the 64 -> 64 layers' padded image is beyond the LDS;
                                     the default learning path in both arms: slab_learning_path does not serve the plane)

    python experiments/step_slab_timing.py [--runs 5] [--workloads ...] [--out FILE]

The driver starts `runs` pairs of fresh child processes per workload, alternating off / on, one after the other, each under its
own `timeout -k 10`; it stops at the first child that does not exit with 0.  A child builds the network, runs the burn-in and 12
warm-up steps, times T net.test steps and T net.learn steps with a host clock around work that ends in a device synchronise, and
then brackets each layer's own step call (Conv2dDCLLlayer's _step with its readouts: the wprep / k_trace launches and the host's
launch gaps included — the same bound for both paths) with device events, 20 calls each.  Ranges are printed, not means; "faster"
is said only where the slow end of the new range beats the fast end of the old one.  Not measured here: DCLL_STEP_SLAB_UNITS other
than 4, and the kernels alone (no profiler run)."""
import argparse
import json
import os
import subprocess
import sys
import time

RADIO = "radio_ml_conv.yaml"
# name -> (spec, plane, batch, readout rows, arp, timed steps, netscale)
WORKLOADS = {"radio-ns3-B64": (RADIO, (16, 16), 64, 24, 1.0, 128, 3.0), "radio-ns3-B128": (RADIO, (16, 16), 128, 24, 1.0, 128, 3.0),
             "radio-ns3-B512": (RADIO, (16, 16), 512, 24, 1.0, 128, 3.0),
             "radio-ns4-B64": (RADIO, (16, 16), 64, 24, 1.0, 128, 4.0), "radio-ns4-B128": (RADIO, (16, 16), 128, 24, 1.0, 128, 4.0),
             "radio-ns4-B512": (RADIO, (16, 16), 512, 24, 1.0, 128, 4.0),
             "radio-ns2-24x40-B64": (RADIO, (24, 40), 64, 24, 1.0, 128, 2.0)}
BURNIN, WARM = 4, 12
CHILD_LIMIT = 300       # seconds, `timeout -k 10` of one child
TAG = "STEP_SLAB_TIMING "


def child(workload, on):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    spec, hw, B, target, arp, steps, netscale = WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    convs = load_network_spec(os.path.join(here, "snn_modulation_classification_amd", "networks", spec))
    args = Namespace(netscale=netscale, alpha=.92, alphas=.85, alpharp=.65, arp=arp, lc_ampl=.5, random_tau=True)
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(args, (1,) + hw, B, convs, target, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam,
                      opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6], burnin=BURNIN)
    net.reset(True)
    net.train()
    slab_learn = net.backward_slab_supported()      # (24x40: no MFMA weight gradient serves the plane; the default one in both arms)
    net.slab_learning_path = slab_learn
    net.slab_step_path = on
    rng = np.random.RandomState(5)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .1).astype(np.float32)).to(dev) for _ in range(8)]
    y = torch.zeros(B, target)
    y[np.arange(B), rng.randint(0, target, size=B)] = 1
    y = y.to(dev)
    rec = dict(workload=workload, on=on, slab_learn=bool(slab_learn), layers=[])
    for name, step in (("learn", lambda x: net.learn(x, y)), ("test", lambda x: net.test(x))):
        for t in range(BURNIN + WARM):
            step(xs[t % 8])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            step(xs[t % 8])
        torch.cuda.synchronize()
        rec[name + "_ms"] = 1e3 * (time.perf_counter() - t0) / steps
    cur = xs[0]
    with torch.no_grad():
        for s in net.dcll_slices:
            L = s.dclllayer
            out = {}
            inp = cur
            call = lambda: L.i2h._step(inp, L.pooling, L.i2o, L.output_ if L.output_layer else None, out=out,
                                       stacked=L.stacked_readout() if L.output_layer else None)
            with ops.kernel_trace() as tr:
                nxt = call()[0].clone()
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            plan = ops.step_slab_plan(L.i2h.make_desc(L.im_dims, L.pooling, L.target_size, L.output_layer), B) if on else None
            rec["layers"].append(dict(kernels=tr.names, us=1e3 * e0.elapsed_time(e1) / 20, plan=plan))
            cur = nxt
    print(TAG + json.dumps(rec))


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

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    for wl in a.workloads:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", wl, "--on", str(on)]
                res = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
                if res.returncode != 0 or not line:         # nothing more is started behind a child that failed
                    flush()
                    sys.exit("child %s on=%d of run %d failed (%d):\n%s" % (wl, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len(TAG):]))
                print("  (%s run %d %s: test %.3f ms, learn %.3f ms)" % (wl, r, "on" if on else "off", rows[-1]["test_ms"], rows[-1]["learn_ms"]),
                      flush=True)
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        say("%s: ms per timestep (%d steps per run, %d alternating fresh processes each, %s in both arms)" %
            (wl, WORKLOADS[wl][5], a.runs, "slab_learning_path on" if rows[0]["slab_learn"] else
             "the default learning path (slab_learning_path does not serve this plane)"))
        for what in ("test", "learn"):
            ms = lambda rs: [x[what + "_ms"] for x in rs]
            say("  net.%-5s default forward " % what + " ".join("%.3f" % v for v in ms(off)) + "   range %.3f .. %.3f" % (min(ms(off)), max(ms(off))))
            say("  net.%-5s slab_step_path  " % what + " ".join("%.3f" % v for v in ms(on)) + "   range %.3f .. %.3f" % (min(ms(on)), max(ms(on))))
            verdict = "faster" if max(ms(on)) < min(ms(off)) else "NOT faster (slower)" if min(ms(on)) > max(ms(off)) else "NOT faster (ranges overlap)"
            say("  net.%s with slab_step_path: %s (%.2fx .. %.2fx)" % (what, verdict, min(ms(off)) / max(ms(on)), max(ms(off)) / min(ms(on))))
        for i in range(len(off[0]["layers"])):
            for name, rs in (("default", off), ("slab", on)):
                us = [x["layers"][i]["us"] for x in rs]
                ks = [k for k in rs[0]["layers"][i]["kernels"]
                      if k.startswith(("k_lif_step", "k_trace", "k_conv_lif", "k_pool", "k_step_wide", "k_step_slab", "k_seq_any"))]
                plan = rs[0]["layers"][i].get("plan")
                say("  layer %d %-8s step call %.1f .. %.1f us   %s%s" % (i, name, min(us), max(us), ", ".join(ks),
                                                                        "" if not plan else "   (bands, slabs) = (%d, %d)" % tuple(plan)))
        say()
        flush()


if __name__ == "__main__":
    main()
