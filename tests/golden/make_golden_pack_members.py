#!/usr/bin/env python3
"""Generates tests/golden/members_*.bin: member frames (include/bwts_members.h) written by the model, tests/pack_members_model.py, from
the members and widths that tests/members_cases.py names.  The suite holds the model to these bytes, so a change of the format
shows."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import members_cases as C  # noqa: E402
import pack_members_model as MM  # noqa: E402


def main():
    for name, (members, widths) in C.fixtures().items():
        frame = MM.pack(members, widths)
        assert MM.unpack(frame) == b"".join(members)
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(frame)
        print("wrote %s: %d bytes for %d in %d members" % (name, len(frame), sum(len(m) for m in members), len(members)))


if __name__ == "__main__":
    main()
