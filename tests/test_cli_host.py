"""acgpt_main's argument handling without a GPU: every case of tests/golden/cli_arguments.json (recorded from the commit before the
query options became a table, by tests/golden/make_cli_golden.py) against the current build.  The arguments are checked before the
device is touched, so a refused text ends with status 2 and the recorded message, and an accepted one gets as far as "Using Direct
Lighting" whether or not a device is there."""
import json
import os
import subprocess

import pytest

import acgpathtracing_amd as pt
from acgpathtracing_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
BOX = os.path.join(pt.SCENES, "cornell_box.obj")
QUERY_OPTIONS = ["--pick", "--pick-all", "--nearest", "--nearest-k", "--within", "--winding", "--clearance", "--tri-distance", "--collide", "--overlap",
                 "--overlap-oriented", "--intersect", "--sweep", "--capsule-cast", "--box-cast", "--cast", "--cast-mesh"]

with open(os.path.join(HERE, "golden", "cli_arguments.json")) as _fh:
    FIXTURE = json.load(_fh)


@pytest.fixture(scope="module")
def exe():
    _build.build_hip()
    return _build.build_main()


def test_fixture_names_every_query_option():
    assert FIXTURE["recorded_from"]
    for option in QUERY_OPTIONS:
        mine = [c for c in FIXTURE["cases"] if c["option"] == option]
        assert all(option in c["args"] for c in mine)
        refused = [c for c in mine if c["refused"] is not None]
        assert len(refused) >= 3 and len(mine) - len(refused) >= 2, option
        assert any(c["args"][-1] == option and c["refused"] == "missing value for %s\n" % option for c in refused), option
        assert any(c["args"][-1] == "" for c in refused), option
        assert option in FIXTURE["gpu_run"]
    assert {c["option"] for c in FIXTURE["cases"]} == set(QUERY_OPTIONS) | {"other"}
    other = [c["args"] for c in FIXTURE["cases"] if c["option"] == "other" and c["refused"] is not None]
    for words in (["--help"], ["--bloom"], ["--ao", "4"], ["--move-history"], ["--error-out", "e.pfm"], ["--denoise", "9"]):
        assert any(a[-len(words):] == words for a in other), words
    assert any(c.get("no_scene") for c in FIXTURE["cases"])


@pytest.mark.parametrize("option", QUERY_OPTIONS + ["other"])
def test_arguments_are_refused_and_accepted_as_recorded(exe, option, tmp_path):
    cases = [c for c in FIXTURE["cases"] if c["option"] == option]
    assert cases
    for c in cases:
        cmd = [exe] + ([] if c.get("no_scene") else ["--obj", BOX]) + c["args"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        if c["refused"] is not None:
            assert r.returncode == 2, (c["args"], r.returncode, r.stderr)
            assert r.stderr == c["refused"], c["args"]
            assert "Using Direct Lighting" not in r.stdout, c["args"]
        else:
            assert r.returncode != 2, (c["args"], r.stderr)
            assert "Using Direct Lighting" in r.stdout, (c["args"], r.stderr)
