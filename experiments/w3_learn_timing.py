"""The per-step timesteps of radio_ml_conv_ref.yaml on the (16,128) plane with ConvNetwork.w3_step_path off (dcll_conv_lif_step's
k_trace + k_conv_lif_tiled<1,3> + k_pool and the generic k_bwd_wgrad — what the parent commit runs, in the same library) and on
(k_lif_step_w3, k_bwd_wgrad_w3), in ms, at B = 64 and B = 512: net.test(x[t]) and net.learn(x[t], y).

    python experiments/w3_learn_timing.py [--runs 5] [--steps 30] [--out FILE]

The driver starts `runs` pairs of fresh child processes per batch size, alternating off / on, each under its own time limit; the
first child that fails ends the run.  A child (at most 16 CPU threads) builds the network, runs the burn-in and warm-up steps of
each kind (a small batch then replays its captured graph, as it defaults), times `steps` steps with a host clock around work that
ends in a device synchronise, and then brackets with device events, 20 calls each,
  - every layer's step call (ops.conv_lif_step without readouts, state advancing), and
  - every slice's open backward call (ops.conv_lif_backward(open_reduce=True): k_bwd_dv + the weight-gradient kernel).
Per layer the table gives, next to the microseconds, the achieved HBM TB/s of the step call against the bytes it has to move
(x, eps0, eps1 in and eps0, eps1 out; arp in and out; v; pooled s and pv — 4 bytes each) and the fraction of the fp32-MFMA peak
(157.3 TFLOP/s) of the step call and of the backward call against 2 x 64 x 3 c_in x h w FLOP per sample each.  Ranges are
printed, not means; the bound for the new path is the default path's own time for the same step."""
import argparse
import json
import os
import subprocess
import sys
import time

HW = (16, 128)
BATCHES = (64, 512)
BURNIN, WARM = 4, 10
KINDS = ("test", "learn")
PEAK_TFLOPS = 157.3


def layer_model(c_in, h, w, B):
    """(bytes the step call moves, FLOP of the chains = FLOP of the weight gradient) of one layer at batch B"""
    n_in, n_out = c_in * h * w, 64 * h * w
    step_bytes = 4 * B * (5 * n_in + 2 * n_out + n_out + 2 * (n_out // 2))
    return step_bytes, 2.0 * B * 64 * 3 * c_in * h * w


def child(B, on, steps):
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
    rec = dict(B=B, on=on, ms={}, layers=[])
    net = None
    for kind in KINDS:
        convs = load_network_spec(os.path.join(here, "snn_modulation_classification_amd", "networks", "radio_ml_conv_ref.yaml"))
        args = Namespace(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
        torch.manual_seed(1)
        np.random.seed(1)
        net = ConvNetwork(args, (1,) + HW, B, convs, 24, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam,
                          opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6], burnin=BURNIN)
        net.reset(True)
        net.w3_step_path = on
        if kind == "test":
            step = lambda t: net.test(xs[t % 4])
        else:
            net.train()
            step = lambda t: net.learn(xs[t % 4], y)
        for t in range(BURNIN + WARM):
            step(t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(steps):
            step(t)
        torch.cuda.synchronize()
        rec["ms"][kind] = 1e3 * (time.perf_counter() - t0) / steps

    def bracket(call, n=20):
        for _ in range(3):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n
    cur = xs[0]
    for s in net.dcll_slices:
        L = s.dclllayer
        i = L.i2h
        desc = i.make_desc(L.im_dims, L.pooling, L.i2o.weight.shape[0], False)
        st = i.state
        out = {}
        call = lambda: ops.conv_lif_step(desc, cur, i.weight, i.bias, i.alpha, i.tau_m__dt, i.alphas, i.tau_s__dt, st.eps0, st.eps1,
                                         st.arp, want_v=True, out=out, w3_path=on)
        with ops.kernel_trace() as tr:
            sp, _, _, pv, v = call()
        us_step = bracket(call)
        g_p = torch.randn(B, 24, device=dev)
        gb = {}
        back = lambda: ops.conv_lif_backward(desc, st.eps1, v, pv, g_p, None, None, None, L.i2o.weight, want_out=False, out=gb,
                                             open_reduce=True, w3_path=on)
        with ops.kernel_trace() as trb:
            back()
        us_back = bracket(back)
        rec["layers"].append(dict(c_in=desc.c_in, h=desc.h, w=desc.w, kernels=tr.names, us=us_step, bwd_kernels=trb.names, bwd_us=us_back))
        cur = sp.clone()
    print("W3_LEARN_TIMING " + json.dumps(rec))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--batches", type=int, nargs="+", default=list(BATCHES))
    p.add_argument("--out")
    p.add_argument("--child", type=int)
    p.add_argument("--on", type=int, default=0)
    a = p.parse_args()
    if a.child:
        return child(a.child, bool(a.on), a.steps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    for B in a.batches:
        rows = []
        for r in range(a.runs):
            for on in (0, 1):
                cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--child", str(B), "--on", str(on),
                       "--steps", str(a.steps)]
                res = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith("W3_LEARN_TIMING ")]
                if res.returncode != 0 or not line:         # (nothing more is started on the device behind a failed child)
                    sys.exit("child B=%d on=%d of run %d failed (%d):\n%s" % (B, on, r, res.returncode, res.stderr[-2000:]))
                rows.append(json.loads(line[0][len("W3_LEARN_TIMING "):]))
        off, on = [x for x in rows if not x["on"]], [x for x in rows if x["on"]]
        say("radio_ml_conv_ref.yaml %dx%d B = %d: timesteps, ms (%d steps per run, %d alternating fresh processes each)"
            % (HW[0], HW[1], B, a.steps, a.runs))
        for kind in KINDS:
            ms = lambda rs: [x["ms"][kind] for x in rs]
            say("  net.%-6s default path  " % kind + " ".join("%.3f" % v for v in ms(off)) + "   range %.3f .. %.3f" % (min(ms(off)), max(ms(off))))
            say("  net.%-6s w3_step_path  " % kind + " ".join("%.3f" % v for v in ms(on)) + "   range %.3f .. %.3f" % (min(ms(on)), max(ms(on))))
            verdict = "faster" if max(ms(on)) < min(ms(off)) else "slower" if min(ms(on)) > max(ms(off)) else "ranges overlap"
            say("  w3_step_path: %s (ratio of the range ends %.2f .. %.2f)" % (verdict, min(ms(off)) / max(ms(on)), max(ms(off)) / min(ms(on))))
        for i, lay in enumerate(off[0]["layers"]):
            nbytes, flop = layer_model(lay["c_in"], lay["h"], lay["w"], B)
            say("  layer %d (%d -> 64 on %dx%d): %.2f MB and %.1f MFLOP per step call" % (i, lay["c_in"], lay["h"], lay["w"], nbytes / 1e6, flop / 1e6))
            for name, rs in (("default", off), ("w3", on)):
                us = [x["layers"][i]["us"] for x in rs]
                bus = [x["layers"][i]["bwd_us"] for x in rs]
                say("    %-8s step call %7.1f .. %7.1f us  %.2f TB/s  %.3f of the fp32-MFMA peak   %s"
                    % (name, min(us), max(us), nbytes / min(us) / 1e6, flop / min(us) / 1e6 / PEAK_TFLOPS, ", ".join(rs[0]["layers"][i]["kernels"])))
                say("    %-8s open backward %7.1f .. %7.1f us  %.3f of the fp32-MFMA peak   %s"
                    % (name, min(bus), max(bus), flop / min(bus) / 1e6 / PEAK_TFLOPS, ", ".join(rs[0]["layers"][i]["bwd_kernels"])))
        say()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
