"""Records tests/golden/query_refusals.json: what the library answers to every case of tests/refusal_cases.py.

    python tests/golden/make_refusals_golden.py [--commit HASH] [--out FILE]

Needs a GPU (pt_create, torch tensors on it) and launches nothing.  Also records what pathtracer.py's wrappers say to a tensor they
refuse (refusal_cases.tensor_messages).  Run it on the build whose refusals are the reference — the commit before a change to
the entry points' argument checks — and name that commit; with another checkout's package first on PYTHONPATH it is that checkout that is recorded.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="", help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "query_refusals.json"))
    args = ap.parse_args()
    import refusal_cases
    from acgpathtracing_amd import _native
    got = refusal_cases.run_all(_native.hip())
    packed = refusal_cases.pack(got)
    with open(args.out, "w") as fh:
        refusal_cases.dump({"recorded_from": args.commit, "answers": packed["answers"], "cases": packed["cases"],
                            "tensor_messages": refusal_cases.run_tensor_messages()}, fh)
    print("%d entry points, %d cases -> %s" % (len(got), sum(len(v) for v in got.values()), args.out))


if __name__ == "__main__":
    main()
