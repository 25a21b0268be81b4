#!/usr/bin/env python3
"""Generates tests/golden/members_v3_mixed.bin: the version-3 member frame (include/bwts_members.h) that the model,
tests/pack_members_v3_model.py, writes of the four members that tests/members_v3_cases.py names -- a chain member, a direct member with
separate planes and a tail, a direct member below the plane minimum, a direct member with the delta filter.  The suite holds the model
and the device to these bytes, so a change of the format shows."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import members_v3_cases as C3  # noqa: E402
import pack_members_v3_model as M3  # noqa: E402


def main():
    members, widths, filters, methods = C3.golden_set()
    frame = M3.pack(members, widths, filters, methods)
    assert M3.unpack(frame) == b"".join(members)
    with open(os.path.join(HERE, C3.GOLDEN), "wb") as f:
        f.write(frame)
    print("wrote %s: %d bytes for %d in %d members" % (C3.GOLDEN, len(frame), sum(len(m) for m in members), len(members)))


if __name__ == "__main__":
    main()
