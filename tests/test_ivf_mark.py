"""S3's k_ivf_mark (fp_kernels.hip: the probed cells' IVF lists read as aligned 16-byte vectors, 4-ary range search per tile,
512-thread workgroups) against numpy on a constructed corpus -- lists of 0 .. 9 entries at every offset modulo 4, the array's
first and last list, a list of more than 4096 entries, one holding every document, lists on either side of a tile boundary;
ivf_mark_worker.py says how the corpus is built and what is compared.  FP_TEST=ivf_tw / ivf_maxcells are read once per process,
so every setting is a subprocess:

  default         the launcher's own tile (one tile at 5000 documents: the filter form), B = 5 with an all-zero query and a subset
  tw16            5000 documents in 12 tiles of 16 words: the search form, B = 3
  tw20            10 tiles of 20 words over W = 192: the last tile overhangs W (tiles of 16 words divide every W, which is a multiple
                  of 64, so the overhang needs a width of its own), B = 1
  tw64            2000 documents, 1152 centroids: one tile, the filter form, n_probe 4
  maxcells3       10 unique cells at 3 per pass: four passes of the chunk loop, the last partial; B = 5 with an all-zero query
  maxcells3_tw16  the same chunk loop in the search form, with a subset

An all-zero query is not marked invalid by the engine (it probes all-tied centroids): its candidates are compared with numpy on
whatever cells the trace returns, and with the oracle modulo those ties."""
import os
import subprocess
import sys

import pytest

import ivf_mark_worker as W
from fptest_env import with_test_opts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(W.CASES))
def test_ivf_mark_against_numpy(case):
    env = with_test_opts(dict(os.environ), **W.CASES[case][0])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ivf_mark_worker.py"), case], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "IVF_MARK_OK" in p.stdout, p.stdout[-4000:]
