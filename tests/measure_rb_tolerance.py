"""Prints the spread the real / bogus GPU tests take their tolerance from: the largest difference in rb between a
float32 and a float64 torch forward on the CPU, over exactly the inputs of each test case (tests/braai_ref.py), and the
bound the GPU is held to (8 x that).  No GPU needed:  python tests/measure_rb_tolerance.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import braai_ref as br  # noqa: E402


def main():
    import torch
    for name, n in (('tiny', 67), ('tiny_wide', 67), ('vgg6', 129)):
        c = br.case(name, n)
        a = br.torch_forward(c['layers'], c['weights'], c['x'], torch.float32)
        b = br.torch_forward(c['layers'], c['weights'], c['x'], torch.float64)
        k = len(c['layers']) - 1
        w32 = c['weights']
        # the logit before the rescaling of the last layer: the spread of the unscaled network
        scale = float(np.abs(np.asarray(w32[-2], np.float64)).max())
        print(f'{name:<10} n = {n:<4} rb span [{c["ref"].min():.4f}, {c["ref"].max():.4f}]  spread fp32 - fp64 = '
              f'{np.abs(a - b).max():.3e}  GPU bound = {c["tol"]:.3e}  (largest last-layer weight {scale:.3g}, '
              f'numpy reference against fp64 torch {np.abs(c["ref"] - b.ravel()).max():.1e})')


if __name__ == '__main__':
    main()
