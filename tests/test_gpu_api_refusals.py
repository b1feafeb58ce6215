"""What the C entry points refuse, and with which words, is what tests/golden/api_refusals.json recorded
(tests/golden/make_golden_api_refusals.py holds the table of calls and says how the file is made)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu


def test_every_entry_point_refuses_and_accepts_what_the_golden_recorded(golden_dir):
    import torch
    from phyloligo_amd import _lib

    spec = importlib.util.spec_from_file_location("make_golden_api_refusals", os.path.join(golden_dir, "make_golden_api_refusals.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(os.path.join(golden_dir, "api_refusals.json")) as fh:
        golden = json.load(fh)
    want = {name: golden["outcomes"][i] for name, i in golden["cases"].items()}
    got = maker.run_cases(_lib.load(), torch)
    assert sorted(got) == sorted(want), "the table of calls and the recorded file name different cases"
    differ = ["%s: recorded %r, now %r" % (name, want[name], got[name]) for name in sorted(want) if got[name] != want[name]]
    assert not differ, "%d of %d calls answer differently:\n%s" % (len(differ), len(want), "\n".join(differ[:40]))
