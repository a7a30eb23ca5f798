"""The learning timestep with ConvNetwork.band_learning_path off (this tree's default weight-gradient dispatch: the generic VALU
k_bwd_wgrad for every layer — the path such a network had before; never the band path itself) and on (k_bwd_wgrad_band: a sample in
bands of conv-output rows), in ms, on planes whose sample no other MFMA weight gradient can stage:

    radio-ns2-24x40-B64, -B512     radio_ml_conv.yaml at netscale 2 on 24x40 (1 -> 64, 64 -> 64, 64 -> 64), slab_step_path on in BOTH arms
    radio-ns1-48x48-B64            radio_ml_conv.yaml at netscale 1 on 48x48 (1 -> 32, 32 -> 32, 32 -> 32), the default forward
    radio-ns2-128x128-B16          radio_ml_conv.yaml at netscale 2 on 128x128, the default forward

    python experiments/bwd_band_timing.py [--runs 5] [--workloads ...] [--bands N] [--out FILE]

--bands N: the "on" arm forces N bands per sample instead of the library's rule.

The driver starts `runs` pairs of fresh child processes per workload, alternating off / on.  A child builds the network, runs the
burn-in and the warm-up learning steps (a small batch then replays its captured graph, as it defaults), times the workload's learning
steps with a host clock around work that ends in a device synchronise, and then brackets each slice's open backward call (dv + weight
gradient, no output_ gradient) with device events, 10 calls each: an UPPER BOUND of the weight-gradient kernel's time that holds the
dv kernel and the host's launch gap too — the same bound for both paths.  Every child also reports the votes of the timed steps (a
hash of every slice's clout): the driver says whether both arms agree.  (The two paths add a row of dW in different orders; both are
within the weight-gradient tolerance of float64, but Adam's normalised update turns a last-bit difference of a near-zero gradient
into a step of +-lr, so free-running arms may part.)  Ranges are printed, not means; "faster" is said only where the slow end of the
new range beats the fast end of the old one, "NOT faster (served)" otherwise.  The launch logs of both arms are printed."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

# workload -> (netscale, plane, B, timed steps, slab_step_path in both arms)
WORKLOADS = {"radio-ns2-24x40-B64": (2.0, (24, 40), 64, 64, True), "radio-ns2-24x40-B512": (2.0, (24, 40), 512, 24, True),
             "radio-ns1-48x48-B64": (1.0, (48, 48), 64, 32, False), "radio-ns2-128x128-B16": (2.0, (128, 128), 16, 12, False)}
SPEC, TARGET, ARP = "radio_ml_conv.yaml", 24, 1.0
BURNIN, WARM = 4, 8
TAG = "BWD_BAND_TIMING "


def child(workload, on, bands):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from argparse import Namespace
    import numpy as np
    import torch
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    netscale, HW, B, STEPS, slab_step = WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    convs = load_network_spec(os.path.join(here, "snn_modulation_classification_amd", "networks", SPEC))
    args = Namespace(netscale=netscale, alpha=.92, alphas=.85, alpharp=.65, arp=ARP, lc_ampl=.5, random_tau=True)
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(args, (1,) + HW, B, convs, TARGET, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam,
                      opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6], burnin=BURNIN)
    net.reset(True)
    net.train()
    if slab_step:
        net.slab_step_path = True
    net.band_learning_path = (bands if bands else True) if on else False
    rng = np.random.RandomState(5)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + HW) < .1).astype(np.float32)).to(dev) for _ in range(8)]
    labels = rng.randint(0, TARGET, size=B)
    y = torch.zeros(B, TARGET)
    y[np.arange(B), labels] = 1
    y = y.to(dev)
    for t in range(BURNIN + WARM):
        net.learn(xs[t % 8], y)
    torch.cuda.synchronize()
    seen = [len(s.clout) for s in net.dcll_slices]
    t0 = time.perf_counter()
    for t in range(STEPS):
        net.learn(xs[t % 8], y)
    torch.cuda.synchronize()
    rec = dict(workload=workload, on=on, steps=STEPS, ms_per_step=1e3 * (time.perf_counter() - t0) / STEPS, layers=[])
    votes = [np.asarray(s.clout)[n:] for s, n in zip(net.dcll_slices, seen)]
    assert all(v.shape == (STEPS, B) for v in votes), [v.shape for v in votes]
    rec["votes"] = hashlib.sha256(b"".join(np.ascontiguousarray(v, dtype=np.int64).tobytes() for v in votes)).hexdigest()
    rec["acc_train"] = [float((v == labels[None, :]).mean()) for v in votes]
    for s in net.dcll_slices:
        L = s.dclllayer
        desc = L.i2h.make_desc(L.im_dims, L.pooling, L.i2o.weight.shape[0], L.output_layer)
        ch, cw, ph, pw = ops.conv_out_shape(desc)
        v = torch.randn(B, L.out_channels, ch, cw, device=dev)
        g_p = torch.randn(B, L.i2o.weight.shape[0], device=dev)
        out = {}
        call = lambda: ops.conv_lif_backward(desc, L.i2h.state.eps1, v, None, g_p, None, None, None, L.i2o.weight, want_out=False, out=out,
                                             open_reduce=True, band_path=on, bands=bands if on else 0)
        with ops.kernel_trace() as tr:
            call()
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            call()
        e1.record()
        torch.cuda.synchronize()
        rec["layers"].append(dict(kernels=tr.names, us=1e3 * e0.elapsed_time(e1) / 10))
    print(TAG + json.dumps(rec))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    p.add_argument("--bands", type=int, default=0)
    p.add_argument("--out")
    p.add_argument("--child")
    p.add_argument("--on", type=int, default=0)
    a = p.parse_args()
    if a.child:
        return child(a.child, bool(a.on), a.bands)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    for wl in a.workloads:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", wl, "--on", str(on), "--bands", str(a.bands)]
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                line = [l for l in res.stdout.splitlines() if l.startswith(TAG)]
                if res.returncode != 0 or not line:
                    sys.exit("child %s on=%d of run %d failed (%d):\n%s" % (wl, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len(TAG):]))
                print("  (%s run %d %s: %.3f ms)" % (wl, r, "on" if on else "off", rows[-1]["ms_per_step"]), flush=True)
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        ms = lambda rs: [x["ms_per_step"] for x in rs]
        say("%s: learning timestep, ms (%d steps per run, %d alternating fresh processes each)%s%s"
            % (wl, off[0]["steps"], a.runs, ", slab_step_path on in both arms" if WORKLOADS[wl][4] else "",
               ", %d bands forced" % a.bands if a.bands else ""))
        say("  default path       " + " ".join("%.3f" % v for v in ms(off)) + "   range %.3f .. %.3f" % (min(ms(off)), max(ms(off))))
        say("  band_learning_path " + " ".join("%.3f" % v for v in ms(on)) + "   range %.3f .. %.3f" % (min(ms(on)), max(ms(on))))
        verdict = "faster" if max(ms(on)) < min(ms(off)) else "NOT faster (served)"
        say("  band path: %s (%.2fx .. %.2fx)" % (verdict, min(ms(off)) / max(ms(on)), max(ms(off)) / min(ms(on))))
        same_votes = len({x["votes"] for x in rows}) == 1
        within = all(len({x["votes"] for x in rs}) == 1 for rs in (off, on))
        say("  votes of the timed steps: %s between the arms (%s among the runs of each arm); acc_train per slice %s (default) / %s (band)"
            % ("EQUAL" if same_votes else "NOT equal", "equal" if within else "NOT equal",
               " ".join("%.4f" % v for v in off[0]["acc_train"]), " ".join("%.4f" % v for v in on[0]["acc_train"])))
        for i in range(len(off[0]["layers"])):
            for name, rs in (("default", off), ("band", on)):
                us = [x["layers"][i]["us"] for x in rs]
                wg = [k for k in rs[0]["layers"][i]["kernels"] if k.startswith("k_bwd_wgrad")]
                say("  layer %d %-8s open backward call (dv + weight gradient) %.1f .. %.1f us   %s" % (i, name, min(us), max(us), ", ".join(wg)))
        say()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
