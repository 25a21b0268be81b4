"""What the suites of the pack that chooses share (include/bwts_members.h, "AUTO"): the eleven 64 KiB inputs of DESIGN section 21 with
their widths, the filter and the method the writer's rules give each (the smallest cell of the section's table), and the model's
answers, made once."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES = 1 << 16

# name, width, the filter and the method that resolve() must name
ROWS = [
    ("int32 random walk", 4, 1, 1),
    ("bf16 gaussian", 2, 0, 1),
    ("f32 gaussian", 4, 0, 1),
    ("f32 smooth (sin)", 4, 1, 0),
    ("int16 sine + noise", 2, 1, 1),
    ("uint64 time stamps", 8, 1, 0),
    ("text (DESIGN.md)", 1, 0, 0),
    ("uniform bytes", 1, 0, None),          # (incompressible: all four cells are the coder's bound, and the tie goes to the chain)
    ("byte ramp", 1, 1, 0),
    ("sorted int32 ids", 4, 1, 1),
    ("f32 random walk", 4, 1, 1),
]
NAMES = [r[0] for r in ROWS]
WIDTHS = [r[1] for r in ROWS]
FILTERS = [r[2] for r in ROWS]
METHODS = [0 if r[3] is None else r[3] for r in ROWS]


@functools.lru_cache(maxsize=None)
def inputs():
    """The eleven inputs as bytes, in the order of ROWS; numpy default_rng(5), drawn in that order."""
    rng = np.random.default_rng(5)
    i = np.arange(BYTES)
    out = [
        np.cumsum(rng.integers(-1000, 1000, BYTES // 4)).astype("<i4"),
        (rng.standard_normal(BYTES // 2).astype("<f4").view("<u4") >> 16).astype("<u2"),
        rng.standard_normal(BYTES // 4).astype("<f4"),
        np.sin(i[:BYTES // 4] * 1e-3).astype("<f4"),
        (8000 * np.sin(i[:BYTES // 2] * 5e-2) + rng.integers(-100, 100, BYTES // 2)).astype("<i2"),
        (1_700_000_000_000_000_000 + np.cumsum(rng.integers(900, 1100, BYTES // 8))).astype("<u8"),
        np.frombuffer(open(os.path.join(ROOT, "DESIGN.md"), "rb").read(BYTES), dtype=np.uint8),
        rng.integers(0, 256, BYTES, dtype=np.uint8),
        (i & 255).astype(np.uint8),
        np.sort(rng.integers(0, 1 << 31, BYTES // 4)).astype("<i4"),
        np.cumsum(rng.standard_normal(BYTES // 4)).astype("<f4"),
    ]
    out = [a.tobytes() for a in out]
    assert all(len(b) == BYTES for b in out)
    return out
