#!/usr/bin/env python3
"""Generates tests/golden/pack_v3_*.bin: version-3 frames (include/bwts_pack.h) written by the model, tests/pack_v3_model.py, from the
inputs, widths and block sizes that tests/test_pack_v3_model.py names.  The suite holds the model to these bytes, so a change of the
format shows."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pack_v3_model as P  # noqa: E402
import test_pack_v3_model as T  # noqa: E402


def main():
    for name, (x, w, B) in T.FIXTURES.items():
        frame = P.pack(x, w, B)
        assert P.unpack(frame) == x
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(frame)
        print("wrote %s: %d bytes for %d" % (name, len(frame), len(x)))


if __name__ == "__main__":
    main()
