"""``activation_special.npz``: every entry of the REFERENCE's ``activation_map``
(cbn/parameter_learning/neural_network.py:10-18, the torch modules themselves)
evaluated on the CPU at float32 special values -- NaN of both signs, +-inf,
+-0, subnormals, +-2^-126, the kernels' tanh branch point 0.625 with its two
float neighbours, the exp clamps 88.7 / 104, 1e30 and FLT_MAX.  Run where the
reference is (never on the GPU box):

    python tests/golden/make_golden_activation.py

tests/test_oracle_golden.py pins ``oracle.ref_infer._act`` to it.  Only the
inputs and outputs land in the fixture; no reference source is copied.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def special_inputs():
    f = np.float32
    nan = f(np.nan)
    sub, tiny, big = f(2.0 ** -149), f(2.0 ** -126), np.finfo(np.float32).max
    b = f(0.625)
    pos = [f(0.0), sub, tiny, np.nextafter(b, f(0)), b, np.nextafter(b, f(1)), f(88.7), f(104.0), f(1e30), big,
           f(np.inf)]
    x = np.array([nan, np.copysign(nan, f(-1))] + [s * v for v in pos for s in (f(1), f(-1))], np.float32)
    assert np.signbit(x[1]) and not np.signbit(x[0]) and np.signbit(x[3]) and x[3] == 0
    return x


def main():
    import torch

    from make_golden_param import _load_reference

    _load_reference()
    from cbn.parameter_learning.neural_network import activation_map

    x = special_inputs()
    out = {"x": x}
    for name, cls in activation_map.items():
        y = cls()(torch.tensor(x)).numpy().astype(np.float32)
        # the values do not depend on the position in the vector or on its
        # length (torch's vectorised loop and its tail): 3 values at a time,
        # in reverse order.  (A ONE-element tensor is different for GELU:
        # nn.GELU()(tensor([inf])) = inf, every longer tensor gives NaN; the
        # reference's hidden layers are [Q, width] tensors, so NaN it is.)
        r = x[::-1].copy()
        one = np.concatenate([cls()(torch.tensor(r[i:i + 3])).numpy() for i in range(0, r.size, 3)])[::-1]
        assert np.array_equal(np.isnan(y), np.isnan(one)) and np.array_equal(
            y[~np.isnan(y)].view(np.uint32), one[~np.isnan(one)].view(np.uint32)), name
        out["y_" + name] = y
        print(name, y)
    np.savez_compressed(os.path.join(HERE, "activation_special.npz"), **out)


if __name__ == "__main__":
    main()
