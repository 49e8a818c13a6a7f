"""Records tests/golden/query_transport_trace.json: what the query wrappers of pathtracer.py send to the library for every case of
tests/transport_cases.py, with a stub in the library's place.

    python tests/golden/make_transport_golden.py [--commit HASH] [--out FILE]

Needs neither a GPU nor a build.  Run it on the commit whose transport is the reference — the one before a change to the wrappers —
and name that commit.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="", help="the commit pathtracer.py is from")
    ap.add_argument("--out", default=os.path.join(HERE, "query_transport_trace.json"))
    args = ap.parse_args()
    import transport_cases
    from acgpathtracing_amd import pathtracer as pt
    got = transport_cases.record(pt)
    from refusal_cases import dump
    with open(args.out, "w") as fh:
        dump(dict(transport_cases.pack(got), recorded_from=args.commit), fh)
    print("%d cases -> %s" % (len(got), args.out))


if __name__ == "__main__":
    main()
