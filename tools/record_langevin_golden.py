"""Record tests/golden/langevin.npz: trajectories of the reference's Langevin samplers (architectures/optimizers.py: SGLD, pSGLD) on the CPU.

    python tools/record_langevin_golden.py /path/to/reference [tests/golden/langevin.npz]

The reference module is loaded by path at run time; none of its text is copied.  Four cases — sgld, sgld_wd, psgld, psgld_wd — each
with parameter tensors of 1, 3, 1025 and 5x3x3x3x3 elements and 4 steps of fixed random gradients.  Before every step torch's CPU
generator is seeded with the recorded per-step seed; the xi of that step are obtained by seeding again and repeating the reference's
draws in its order (SGLD: torch.randn_like(p); pSGLD: torch.empty(shape).normal_(), what p.new(size).normal_() does), and the recorder
checks that a restatement of the update with those xi lands within rounding of what the reference produced.

Keys: "<case>/hyper" (JSON string), "<case>/seeds" (int64[steps]), "<case>/p<i>_init", and per step s and tensor i
"<case>/g<s>_<i>", "<case>/xi<s>_<i>", "<case>/p<s>_<i>", "<case>/V<s>_<i>" (V only for pSGLD).  CPU only, no GPU needed.
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

SHAPES = [(1,), (3,), (1025,), (5, 3, 3, 3, 3)]
STEPS = 4
CASES = {
    "sgld": dict(kind="sgld", lr=0.01, weight_decay=0.0, noise_scale=0.1),
    "sgld_wd": dict(kind="sgld", lr=0.01, weight_decay=0.05, noise_scale=0.1),
    "psgld": dict(kind="psgld", lr=0.01, weight_decay=0.0, beta=0.99, Lambda=1e-8),
    "psgld_wd": dict(kind="psgld", lr=0.01, weight_decay=0.05, beta=0.99, Lambda=1e-8),
}


def load_reference(root):
    spec = importlib.util.spec_from_file_location("_ref_optimizers", os.path.join(root, "architectures", "optimizers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw(kind, p):
    return torch.randn_like(p) if kind == "sgld" else torch.empty(p.shape, dtype=torch.float32).normal_(mean=0, std=1)


def record_case(ref, name, hyper, out):
    rng = np.random.RandomState(sum(map(ord, name)))
    kind = hyper["kind"]
    params = [torch.nn.Parameter(torch.from_numpy((0.1 * rng.randn(*s)).astype(np.float32))) for s in SHAPES]
    for i, p in enumerate(params):
        out["%s/p%d_init" % (name, i)] = p.detach().numpy().copy()
    if kind == "sgld":
        opt = ref.SGLD(params, lr=hyper["lr"], weight_decay=hyper["weight_decay"], noise_scale=hyper["noise_scale"])
    else:
        opt = ref.pSGLD(params, lr=hyper["lr"], beta=hyper["beta"], Lambda=hyper["Lambda"], weight_decay=hyper["weight_decay"])
    seeds = [int(rng.randint(1, 2 ** 31 - 1)) for _ in range(STEPS)]
    for s in range(STEPS):
        grads = [(0.02 * rng.randn(*sh)).astype(np.float32) for sh in SHAPES]
        before = [p.detach().clone() for p in params]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        torch.manual_seed(seeds[s])
        opt.step()
        torch.manual_seed(seeds[s])
        for i, (p, g) in enumerate(zip(params, grads)):
            xi = draw(kind, p)
            out["%s/g%d_%d" % (name, s, i)] = g
            out["%s/xi%d_%d" % (name, s, i)] = xi.numpy().copy()
            out["%s/p%d_%d" % (name, s, i)] = p.detach().numpy().copy()
            d = torch.from_numpy(g) + hyper["weight_decay"] * before[i]
            if kind == "psgld":
                V = opt.state[p]["V"]
                out["%s/V%d_%d" % (name, s, i)] = V.numpy().copy()
                G = V.sqrt() + hyper["Lambda"]
                want = before[i] - hyper["lr"] * d / G + xi * (2 * hyper["lr"] / G).sqrt()
            else:
                want = before[i] - hyper["lr"] * d + float(np.sqrt(hyper["noise_scale"])) * xi
            # the re-seeded draws are the ones the reference consumed: a wrong xi would be off by O(noise), not by roundings
            assert torch.allclose(want, p.detach(), rtol=1e-5, atol=1e-6), (name, s, i)
    out[name + "/hyper"] = np.array(json.dumps(hyper))
    out[name + "/seeds"] = np.array(seeds, dtype=np.int64)


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    warnings.filterwarnings("ignore")
    ref = load_reference(argv[1])
    path = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "langevin.npz")
    out = {}
    for name, hyper in CASES.items():
        record_case(ref, name, hyper, out)
    out["cases"] = np.array(list(CASES))
    out["shapes"] = np.array(json.dumps(SHAPES))
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv)
