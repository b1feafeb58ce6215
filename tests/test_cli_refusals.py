"""The command line's one parser, one rule table and one launch decision, on the CPU.

tests/golden/cli_refusals.json (tests/golden/make_golden_cli_refusals.py) records, for a product of modes, containers, metrics,
GPU counts, methods and clip options, the first reason the CLI gave for refusing each command line before the refusal rules were
gathered into one table; the rules must give the same text, to the byte, for every one of them."""
import itertools
import json
import os
import subprocess
import sys

import pytest

from phyloligo_amd import phyloligo as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["-i", "x.fa", "--method", "joblib"]


def test_recorded_refusals_replay(golden_dir, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with open(os.path.join(golden_dir, "cli_refusals.json")) as fh:
        rec = json.load(fh)
    lines = [["-i", "x.fa"] + [w for part in parts for w in part] for parts in itertools.product(*rec["factors"].values())]
    assert len(lines) == len(rec["index"]) >= 6000 and len(rec["messages"]) >= 40
    assert sorted(set(rec["index"])) == list(range(len(rec["messages"])))
    for argv, k in zip(lines, rec["index"]):
        params = P.get_cmd(argv)
        want = rec["messages"][k]
        assert P.refusal(params) == want, argv
        if "--gpus" in argv:             # what the process that would start the ranks says, before it starts any
            assert P.launch_plan(params, {})[:2] == (want, 2), argv
        if want is not None:
            with pytest.raises(SystemExit) as e:
                P.refuse(P.refusal(params), speak=False)
            assert e.value.code == 1


def test_refuse_speaks_once_on_stderr(capsys):
    P.refuse(None)
    with pytest.raises(SystemExit) as e:
        P.refuse("Error, no")
    assert e.value.code == 1 and capsys.readouterr() == ("", "Error, no\n")
    with pytest.raises(SystemExit):
        P.refuse("Error, no", speak=False)
    assert capsys.readouterr() == ("", "")


def test_launch_plan_sees_abbreviated_options():
    """argparse accepts unambiguous prefixes; the decision is taken from what it parsed, so they count like the full spelling"""
    refused, gpus, _ = P.launch_plan(P.get_cmd(BASE + ["--gp", "2", "--tsne", "30"]), {})
    assert gpus == 2 and refused == "Error, --tsne runs on one GPU: an embedding over several ranks (--gpus N > 1) is out of scope"
    assert refused == P._tsne_refused(P.get_cmd(BASE + ["--gpus", "2", "--tsne", "30"]))
    for extra in (["--kmedoids-s", "2:3"], ["--clip-p", "0.9"], ["--min-s", "5"], ["--kmedoids", "3"], ["--clip-percentile=0.5"]):
        assert P.launch_plan(P.get_cmd(BASE + extra), {}) == (None, 1, True), extra
    for extra in ([], ["--knn", "8"], ["--tsne", "30"], ["--tsne-s", "3", "--tsne", "30"], ["--large", "memmap"],
                  ["--clip-percentile", "1", "--min-size", "0"]):
        assert P.launch_plan(P.get_cmd(BASE + extra), {}) == (None, 1, False), extra
        assert P.launch_plan(P.get_cmd(BASE + extra), {"WORLD_SIZE": "2"})[2] is True, extra
    assert P.launch_plan(P.get_cmd(BASE), {"WORLD_SIZE": "1"})[2] is False
    # a rank is refused what the process that starts the ranks is refused
    assert "--kmedoids runs on one GPU" in P.launch_plan(P.get_cmd(BASE + ["--kmedoids", "3"]), {"WORLD_SIZE": "2"})[0]


def test_refused_process_exits_1_without_torch(tmp_path):
    """`python -m phyloligo_amd` parses, decides and refuses without importing torch, also for a mode that would need it"""
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGTACGTAC\n>b\nACGTTTGCAA\n")
    args = ["-i", str(fa), "--method", "joblib", "--kmedoids", "2", "--large", "memmap", "-o", str(tmp_path / "c.txt")]
    code = ("import sys, runpy\n"
            "sys.argv = ['phyloligo_amd'] + %r\n"
            "try:\n    runpy.run_module('phyloligo_amd', run_name='__main__')\n"
            "except SystemExit as e:\n    print('EXIT', e.code)\n"
            "print('TORCH_IMPORTED' if 'torch' in sys.modules else 'NO_TORCH')\n") % (args,)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["EXIT", "1", "NO_TORCH"]
    assert out.stderr == ("Error, --kmedoids writes one label per contig as text, not a matrix container: it cannot be combined with "
                          "--large memmap\n")
    assert not (tmp_path / "c.txt").exists()
    plain = subprocess.run([sys.executable, "-m", "phyloligo_amd"] + args, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert plain.returncode == 1 and plain.stdout == "" and plain.stderr == out.stderr
