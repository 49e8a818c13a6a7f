"""Every query option of acgpt_main in one run on the Cornell box, each in a form that finds something and a form that finds nothing:
the JSON lines it prints, in order, against tests/golden/cli_queries_stdout.txt byte for byte.  The file was recorded from the commit
before the query options became a table (tests/golden/make_cli_golden.py --gpu, which ran that binary twice and found the same
bytes: the queries use no atomics).  The command line is the fixture's "gpu_run"; the mesh of --collide and --cast-mesh is
tests/golden/cli_ball.obj, named by a relative path so that the printed path is the same everywhere."""
import json
import os
import subprocess

import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _native

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOX = os.path.join(pt.SCENES, "cornell_box.obj")


def test_cli_query_lines_are_the_recorded_bytes(built, tmp_path):
    exe = os.path.join(os.path.dirname(_native.hip_library_path()), "acgpt_main")
    with open(os.path.join(GOLDEN, "cli_arguments.json")) as fh:
        args = json.load(fh)["gpu_run"]
    assert args[:8] == ["--width", "8", "--height", "8", "--spp-per-launch", "1", "--frames", "1"]
    run = subprocess.run([exe, "--obj", BOX] + args + ["--out", str(tmp_path / "frame.png")], capture_output=True, cwd=GOLDEN, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    got = [l for l in run.stdout.split(b"\n") if l.startswith(b"{")]
    with open(os.path.join(GOLDEN, "cli_queries_stdout.txt"), "rb") as fh:
        want = fh.read().split(b"\n")[:-1]
    assert len(want) == sum(a.startswith("--") and a not in ("--width", "--height", "--spp-per-launch", "--frames", "--zoom") for a in args)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert len(got) == len(want)
    assert (tmp_path / "frame.png").exists()
