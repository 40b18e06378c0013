"""
Host-independent initial weights for the long-horizon GPU parity tests.

The product initialises its networks on the host with nn.init.orthogonal_: a float32 LAPACK QR of a seeded Gaussian
matrix.  The Gaussian draws are the same everywhere, but the QR's last bits depend on the BLAS build, the CPU and
the number of intra-op threads.  Tests that compare tens to a thousand sequential Adam steps of two float32
computations (the GPU path against the CPU port, or two GPU chains that sum in different orders) drift apart by
amounts that depend on where they start, so they must start from the same weights on every host.

  float64_orthogonal_init()  networks built inside the block draw the same Gaussian matrices and factor them in
                             float64; rounded to float32, the weights no longer depend on how the QR was computed.
  load_c1_weights(ppo)       C1 (tests/test_gpu_end_to_end.py::test_c1_config_two_full_iterations_match_cpu_port)
                             starts from the weights its tolerances were set on: tests/golden/g15_c1_initial_weights.npz,
                             the float32 draw of torch 2.10 (MKL) on an AMD EPYC 9575F host with 128 intra-op threads
                             (record_c1_weights() on such a host).  From the float64 draw, the torch update mode's
                             critic ends its 80 Adam steps with 23 % of its weights more than 3e-5 from the CPU port's
                             (bound: 1 %); from the stored weights, under 1 %.
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
C1_WEIGHTS = os.path.join(os.path.dirname(HERE), "golden", "g15_c1_initial_weights.npz")


def _orthogonal_float64_(tensor, gain=1, generator=None):
    """nn.init.orthogonal_ with the QR and the gain in float64, rounded once to the tensor's dtype."""
    rows = tensor.size(0)
    cols = tensor.numel() // rows
    flattened = tensor.new_empty((rows, cols)).normal_(0, 1, generator=generator)
    if rows < cols:
        flattened.t_()
    q, r = torch.linalg.qr(flattened.double())
    q *= torch.diag(r, 0).sign()
    if rows < cols:
        q.t_()
    with torch.no_grad():
        tensor.view_as(q).copy_(q * gain)
    return tensor


@contextlib.contextmanager
def float64_orthogonal_init():
    """Networks built inside the block are initialised by _orthogonal_float64_ (same draws, same generator)."""
    orig = torch.nn.init.orthogonal_
    torch.nn.init.orthogonal_ = _orthogonal_float64_
    try:
        yield
    finally:
        torch.nn.init.orthogonal_ = orig


def load_c1_weights(ppo):
    """Overwrite policy "p"'s freshly initialised actor + critic bucket with the stored C1 weights."""
    w = np.load(C1_WEIGHTS, allow_pickle=False)["policy"]
    with torch.no_grad():
        ppo.policies["p"].policy_params.copy_(torch.from_numpy(w))


def record_c1_weights(threads=128):
    """Recipe of g15_c1_initial_weights.npz: the C1 trainer as the test builds it, drawn with `threads` threads."""
    sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]     # tests/, the repository
    from test_gpu_end_to_end import _make
    saved = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        ppo = _make(8, 128, 256, 10, term_prob=0.02, max_ts=200)
    finally:
        torch.set_num_threads(saved)
    np.savez_compressed(C1_WEIGHTS, policy=ppo.policies["p"].policy_params.cpu().numpy())


if __name__ == "__main__":
    record_c1_weights()
