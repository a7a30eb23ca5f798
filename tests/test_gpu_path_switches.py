"""Launch sequences and parameter bits of every combination of the opt-in path switches the setters accept.

mnist_conv.yaml (it pools, so pool_dv_path does something) at netscale 1 and 2 — at 2 the `any` paths refuse and the `wide` kernels run —
under every step path x learning path x pool_dv_path, and radio_ml_conv_ref.yaml on (16, 128) under w3_step_path x w3_first_wgrad x
w3_dv_path; B = 2, no captured graphs, burn-in 2.  A cell is four net.learn steps and two net.test steps under ops.kernel_trace; the
kernel names and a SHA-256 of all parameters and buffers afterwards are compared with tests/path_launch_expected.json, which
`python tests/test_gpu_path_switches.py FILE COMMIT` recorded (twice, the two agreeing) at the commit it names — the one before the path
registry, on which this module runs unmodified.  A refused combination is recorded as such.
"""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
EXPECTED = os.path.join(ROOT, "tests", "path_launch_expected.json")
pytestmark = pytest.mark.gpu

STEP = [None, "any_step_path", "wide_step_path", "slab_step_path"]
LEARNING = [None, ("any_learning_path", True), ("wide_learning_path", True), ("slab_learning_path", True), ("band_learning_path", True),
            ("band_learning_path", 2)]
# group -> (yaml, plane, netscale, classes, the settings of each cell)
GROUPS = {
    "mnist_ns1": ("mnist_conv.yaml", (28, 28), 1.0, 10, None),
    "mnist_ns2": ("mnist_conv.yaml", (28, 28), 2.0, 10, None),
    "ref_w3": ("radio_ml_conv_ref.yaml", (16, 128), 1.0, 24,
               [[(n, True) for n, on in zip(("w3_step_path", "w3_first_wgrad", "w3_dv_path"), bits) if on]
                for bits in itertools.product((0, 1), repeat=3)]),
}
MNIST_CELLS = [([(s, True)] if s else []) + ([l] if l else []) + ([("pool_dv_path", True)] if dv else [])
               for s, l, dv in itertools.product(STEP, LEARNING, (0, 1))]


def cells(group):
    return GROUPS[group][4] or MNIST_CELLS


def label(settings):
    return ", ".join("%s=%s" % s for s in settings) or "default"


def run_cell(group, settings, dev):
    """-> 'refused: <class>' where a setter refuses, else [kernel names, sha256 of the state dict]"""
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    from argparse import Namespace
    yaml, hw, netscale, target, _ = GROUPS[group]
    B = 2
    torch.manual_seed(1)
    np.random.seed(1)
    args = Namespace(netscale=netscale, alpha=.92, alphas=.85, alpharp=.65, arp=0.0, lc_ampl=.5, random_tau=True)
    net = ConvNetwork(args, (1,) + hw, B, load_network_spec(os.path.join(PKG, "networks", yaml)), target, act=torch.nn.Sigmoid(),
                      loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam, opt_param={"betas": [0.0, .95], "weight_decay": 10.0},
                      learning_rates=[1e-6], burnin=2)
    net.graph_learn = False
    net.reset(True)
    net.train()
    for name, value in settings:
        try:
            setattr(net, name, value)
        except Exception as e:
            return "refused: " + type(e).__name__
        assert getattr(net, name) == value
    rng = np.random.RandomState(7)
    y = torch.zeros(B, target)
    y[np.arange(B), rng.randint(0, target, size=B)] = 1
    y = y.to(dev)
    x = [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .15).astype(np.float32)).to(dev) for _ in range(6)]
    with ops.kernel_trace() as tr:
        for t in range(4):
            net.learn(x[t], y)
        net.eval()
        for t in range(4, 6):
            net.test(x[t])
        torch.cuda.synchronize()
    h = hashlib.sha256()
    for k, v in sorted(net.state_dict().items()):
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return [list(tr.names), h.hexdigest()]


def run_group(group):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    return {label(s): run_cell(group, s, dev) for s in cells(group)}


def pack(recorded_at, groups):
    """The recording as the text of tests/path_launch_expected.json: the distinct kernel names, the distinct launch logs as indices
    into them (one line each), and one line per cell: 'refused: <class>' or [index of its log, sha256]."""
    names = sorted({n for g in groups.values() for v in g.values() if not isinstance(v, str) for n in v[0]})
    logs = sorted({tuple(names.index(n) for n in v[0]) for g in groups.values() for v in g.values() if not isinstance(v, str)})
    out = ['{"recorded_at": %s,' % json.dumps(recorded_at), '"kernels": %s,' % json.dumps(names), '"logs": [']
    out += ['%s,' % json.dumps(list(l)) for l in logs]
    out[-1] = out[-1][:-1] + '],'
    out.append('"groups": {')
    for g, cells_ in sorted(groups.items()):
        out.append('%s: {' % json.dumps(g))
        for k, v in sorted(cells_.items()):
            out.append('%s: %s,' % (json.dumps(k), json.dumps(v if isinstance(v, str) else
                                                              [logs.index(tuple(names.index(n) for n in v[0])), v[1]])))
        out[-1] = out[-1][:-1] + '},'
    out[-1] = out[-1][:-1] + '}}'
    return "\n".join(out) + "\n"


def unpack(text):
    """pack's text -> {group: {cell: 'refused: <class>' or [kernel names, sha256]}}, what run_group returns per group"""
    doc = json.loads(text)
    return {g: {k: v if isinstance(v, str) else [[doc["kernels"][i] for i in doc["logs"][v[0]]], v[1]] for k, v in c.items()}
            for g, c in doc["groups"].items()}


@pytest.mark.parametrize("group", list(GROUPS))
def test_launch_log_and_parameter_bits_of_every_accepted_combination(group):
    with open(EXPECTED) as f:
        want = unpack(f.read())[group]
    got = run_group(group)
    assert set(got) == set(want) and len(got) == len(cells(group))
    ran = [k for k, v in want.items() if not isinstance(v, str)]
    assert len(ran) == {"mnist_ns1": 48, "mnist_ns2": 30, "ref_w3": 5}[group]       # (what the switches' own rules leave)
    for k in sorted(want):
        if isinstance(want[k], str):
            assert got[k] == want[k], k
            continue
        assert not isinstance(got[k], str), (k, got[k])
        assert got[k][0] == want[k][0], "launch log of [%s]:\n%s\nrecorded:\n%s" % (k, got[k][0], want[k][0])
        assert got[k][1] == want[k][1], "parameter bits of [%s]" % k


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    groups = {g: run_group(g) for g in GROUPS}
    text = pack("commit %s, by tests/test_gpu_path_switches.py" % sys.argv[2], groups)           # FILE COMMIT
    assert unpack(text) == groups
    with open(sys.argv[1], "w") as f:
        f.write(text)
