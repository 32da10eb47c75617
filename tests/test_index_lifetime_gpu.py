"""The life of an fp_index on the device (fp_index.cpp): refusals of fp_index_create after device work has begun, every branch of
the layout code read back through fp_index_export / fp_index_read_doc / fp_index_read_ivf, 20 create / destroy rounds of each
index, and fp_index_device_bytes / fp_index_num_code_lines against recorded values.  One run of index_lifetime_worker.py (which
describes the groups and asserts them) serves the three tests."""
import json
import os
import subprocess
import sys

import pytest

import index_lifetime_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> [fp_index_device_bytes, fp_index_num_code_lines].  Recorded by running the worker once on the MI355X against the library
# of the commit BEFORE index construction moved to fp_index.cpp (FP_LIB_PATH): the move must not change what an index counts.
FIGURES = {
    "native128": [579824, 0],
    "padded96": [516176, 0],
    "sliced40": [223450, 0],
    "lines8": [20185972, 364],
    "empty": [11233, 0],
    "synthetic": [657528, 0],
}


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("index_lifetime") / "out.json")
    env = dict(os.environ)
    env.pop("FP_APPROX_IMPL", None)   # (the packed code lines of "lines8" come from the index's own predicate)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "index_lifetime_worker.py"), out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert os.path.exists(out), p.stdout[-4000:]
    with open(out) as f:
        return json.load(f)


def test_refusals_after_device_work_has_begun(verdicts):
    assert verdicts["refusals"] == "ok", verdicts["refusals"]
    assert verdicts["searched"] > 0


def test_layout_branches_read_back_and_recreate(verdicts):
    assert verdicts.get("layouts") == "ok", verdicts.get("layouts", "not run: the refusal group failed")


def test_device_bytes_and_code_lines(verdicts):
    assert set(FIGURES) == set(W.CONFIGS) | {"synthetic"}
    assert verdicts.get("figures") == FIGURES
    assert FIGURES["lines8"][1] > 0
