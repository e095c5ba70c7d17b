"""Writes conv_nt24.npz: the convolution objective at nt = 24 from the dense restatement (tests/conv_ref.py).

κ (column 1 of the dense K below its first row), fvec, the scalars T0 / T1, 5 integer controls in -2..2 and the
restatement's J and df for each.  Run from the repository root: python tests/golden/conv/make_conv_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from conv_ref import ConvRef, controls  # noqa: E402


def main():
    nt = 24
    ref = ConvRef(nt)
    xs = controls(nt, 5, seed=24)
    np.savez(os.path.join(HERE, "conv_nt24.npz"), scalars=np.array([ref.T0, ref.T1]), kappa=ref.K[1:, 0].copy(),
             fvec=ref.fvec, x=np.stack(xs), J=np.array([ref.eval_f(x) for x in xs]),
             df=np.stack([ref.eval_df(x) for x in xs]))


if __name__ == "__main__":
    main()
