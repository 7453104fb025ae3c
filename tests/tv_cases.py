"""The total-variation cases shared by tests/golden/make_golden_tv.py, tests/test_tv_host.py and tests/test_gpu_tv.py: names, seeds, shapes, dtypes, and the
inputs regenerated from the seeds (the fixture g17_tv.npz stores values and gradients only)."""
import numpy as np
import torch

# name, seed, shape, dtype, what it pins
CASES = [
    ("s5437", 1700, (5, 4, 3, 7), "f32"),          # unequal extents pin the /shape[0] rule; C odd
    ("s2221", 1701, (2, 2, 2, 1), "f32"),          # smallest input with a difference on every axis
    ("s3142", 1702, (3, 1, 4, 2), "f32"),          # an axis of extent 1
    ("s331796", 1703, (33, 17, 9, 6), "f32"),      # more than one workgroup: the partials pass
    ("s99948", 1704, (9, 9, 9, 48), "f32"),        # the grid's width
    ("s666200_bf16", 1705, (6, 6, 6, 200), "bf16"),     # the instance head's width and dtype
    ("s666200_f16", 1705, (6, 6, 6, 200), "f16"),
    ("s81", 1706, (8, 1), "f32"),                  # rank 2
    ("s321", 1707, (3, 2, 1), "f32"),              # rank 3
    ("s4445_const", 1708, (4, 4, 4, 5), "f32"),    # a constant 2x2x2x5 block: exact-zero differences, sign(0) = 0
]
GRAD_CASES = ("s5437", "s2221", "s3142", "s99948", "s4445_const")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

GRID_SEED, GRID_N, GRID_SAMPLE_SIZE = 1, 4, 0.2
GRID_A = np.array([[0.7, -0.3, 0.2, 1.1, -0.9], [0.4, 0.8, -0.6, 0.1, 0.5], [-0.2, 0.6, 0.9, -0.7, 0.3]], np.float32)
GRID_B = np.array([0.1, -0.2, 0.3, 0.0, 0.5], np.float32)


def case_values(seed, shape, dtype, const_block=False):
    """The case's input as a CPU tensor of its dtype: standard normal from np.random.RandomState(seed), rounded once to the dtype."""
    x = np.random.RandomState(seed).standard_normal(size=shape).astype(np.float32)
    if const_block:
        x[1:3, 1:3, 1:3, :] = 0.5
    return torch.from_numpy(x).to(DTYPES[dtype])


def case(name):
    for n, seed, shape, dtype in CASES:
        if n == name:
            return case_values(seed, shape, dtype, n.endswith("_const"))
    raise KeyError(name)


def grid_encoder(seen=None):
    """sin of a fixed linear map of the coordinates: [K,1,3] -> [K,1,5]; appends the coordinates it received to `seen`."""
    A, b = torch.from_numpy(GRID_A), torch.from_numpy(GRID_B)

    def enc(coords):
        if seen is not None:
            seen.append(coords.detach().cpu().clone())
        return torch.sin(coords @ A.to(coords.device) + b.to(coords.device))
    return enc
