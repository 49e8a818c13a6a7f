"""Records tests/golden/cast_walk.npz: what the sweep, capsule, box and triangle casts and pt_query_poses_cast answer to every case of
tests/cast_walk_cases.py: records, any-hit bytes and the visit pairs of every mode of the pt_debug_*_visits hooks, on four scenes under
both node formats.

    python tests/golden/make_cast_walk_golden.py --commit HASH [--out FILE]

Needs a GPU.  Run it on the build whose answers are the reference, the commit before a change to the casts' walk, and name that
commit.  The committed file was recorded from ecea533, the parent of the commit that introduced csrc/cast_walk.h.  The inputs are not
stored: cast_walk_cases regenerates them from its seeds, and tests/test_cast_walk_host.py holds the recorded records to the CPU
references.  The script refuses to write a file in which one (family, scene) has different records under two formats, calls or modes.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "cast_walk.npz"))
    args = ap.parse_args()
    import numpy as np
    import cast_walk_cases as cw
    got = cw.run_all()
    assert sorted(got) == sorted(cw.all_keys())
    packed = cw.pack(got)
    np.savez_compressed(args.out, recorded_from=np.array(args.commit), **packed)
    print("%d outputs, %d arrays, %d bytes -> %s" % (len(got), len(packed), os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
