"""Record the fixtures of --net attmultiunet by RUNNING THE REFERENCE on the CPU (build container only, like oracle/make_golden.py):

    python tools/make_golden_attention.py

  tests/golden/attention.npz
    gate2d          the reference's GridAttentionBlock(6, 5, 4): forward, input and parameter gradients, running statistics
    net2d_bilinear  the reference's AttMulResUnet2D(6 -> 2, [4, 4, 8, 8, 8]) on (1, 6, 32, 48): key list, forward, all gradients
    net2d_nearest   the same with nearest-neighbour up-sampling in the decoder (the gates stay bilinear)
  tests/golden/net_attmultiunet25d_tiny.npz
    six iterations of the reference's Interpolator with --datadim 2.5d --net attmultiunet on a 48 x 32 x 3 slab (a size at which the
    reference's loss history does not depend on its summation order to 1e-5; 64 x 32 x 3 with nearest up-sampling does, to 5e-3)

The recording helpers, the synthetic data and the thread count are those of oracle/make_golden.py; the reference is imported through
oracle/ref_shim.py.  The committed .npz files hold data only.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from oracle.make_golden import THREADS, grads_np, hyperbolic_volume, run_reference_interpolator, save, sd_np, trace_mask  # noqa: E402


def key_list(module):
    return json.dumps([[k, list(v.shape)] for k, v in module.state_dict().items()])


def seeded(make):
    """set_seed(0) + construction + init_weights(xavier, 0.02): the state the reference's Interpolator starts from."""
    import utils as u
    u.set_seed(0)
    m = make()
    u.init_weights(m, "xavier", 0.02)
    return m


def gen_gate():
    from architectures.attention import GridAttentionBlock
    gen = torch.Generator().manual_seed(2024)
    m = seeded(lambda: GridAttentionBlock(6, 5, 4))
    d = {"state": sd_np(m)}
    g = torch.randn((1, 6, 3, 5), generator=gen).requires_grad_(True)
    x = torch.randn((1, 5, 6, 10), generator=gen).requires_grad_(True)
    y = m(g, x)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    d.update({"g": g, "x": x, "y": y, "dy": dy, "dg": g.grad, "dx": x.grad, "grads": grads_np(m), "state_after": sd_np(m)})
    return d


def gen_net(mode):
    from architectures.attention import AttMulResUnet2D
    gen = torch.Generator().manual_seed(12 if mode == "bilinear" else 7)
    m = seeded(lambda: AttMulResUnet2D(num_input_channels=6, num_output_channels=2, num_channels_down=[4, 4, 8, 8, 8], upsample_mode=mode))
    d = {"keys": key_list(m), "init_state": sd_np(m)}
    x = torch.randn((1, 6, 32, 48), generator=gen).requires_grad_(True)
    y = m(x)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    d.update({"x": x, "y": y, "dy": dy, "dx": x.grad, "grads": grads_np(m)})
    return d


def main():
    torch.set_num_threads(THREADS)
    ref_shim.install()
    save("attention", {"gate2d": gen_gate(), "net2d_bilinear": gen_net("bilinear"), "net2d_nearest": gen_net("nearest")})
    vol = hyperbolic_volume((48, 32, 3), seed=9)
    msk = trace_mask((48, 32, 3), 0.5, seed=10)
    save("net_attmultiunet25d_tiny",
         run_reference_interpolator(["--imgdir", "/nonexistent", "--datadim", "2.5d", "--net", "attmultiunet", "--filters", "4", "4", "8", "8", "8",
                                     "--inputdepth", "6", "--upsample", "linear", "--gain", "1"], vol * 1.0, msk, 6, "2.5d attention"))


if __name__ == "__main__":
    main()
