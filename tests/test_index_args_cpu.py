"""CPU tests (no GPU) of the refusals of index construction and read-back (fp_index.cpp) that happen before the device is touched:
fp_index_create, fp_index_create_synthetic, and fp_index_read_doc / fp_index_read_ivf / fp_index_ivf_total / fp_index_export / the
getters on a null index.  Each case asserts the return code and the exact fp_last_error() text, read off the validation code, and
that *out is null afterwards.  The library loads without a GPU, and no case here starts one."""
import ctypes

import numpy as np
import pytest

FP_OK, FP_EINVAL, FP_EHIP, FP_EUNSUPPORTED = 0, -1, -3, -4
NBITS = "nbits must divide 8 (1, 2, 4 or 8)"
DIM = "dim must be a multiple of 8 in [8, 1024]"
SENTINEL = 0xDEAD0   # what *out holds before a call that has to clear it

GETTERS = ("fp_index_num_docs", "fp_index_num_tokens", "fp_index_num_centroids", "fp_index_dim", "fp_index_nbits",
           "fp_index_device_bytes", "fp_index_num_unique_codes", "fp_index_num_code_lines", "fp_index_num_hard_tokens",
           "fp_index_tickets_ok")


def _addr(a):
    return None if a is None else a.ctypes.data


def _desc(nbits=4, dim=8, C=2, n_docs=1, **missing):
    """a valid descriptor of one document of two tokens (arrays kept alive on the returned object); `missing` names the
    fields to null"""
    from fast_plaid_amd import _native
    pr = max(dim * nbits // 8, 1)
    keep = dict(centroids=np.zeros((C, max(dim, 1)), np.float16), bucket_weights=np.zeros(1 << nbits, np.float16),
                doc_codes=np.zeros(2, np.int64), doc_residuals=np.zeros((2, pr), np.uint8), doc_lengths=np.array([2], np.int64))
    d = _native.FpIndexDesc(nbits=nbits, dim=dim, n_centroids=C, n_docs=n_docs, n_ivf_lists=0, pid_offset=0)
    for k, v in keep.items():
        setattr(d, k, None if missing.get(k) else _addr(v))
    d._keep = keep
    return d


def _synth(nbits=4, dim=8, C=2, total=4, begin=0, end=4, doc_len=3):
    from fast_plaid_amd import _native
    keep = (np.zeros((max(C, 1), max(dim, 1)), np.float16), np.zeros(1 << nbits, np.float16))
    d = _native.FpSynthDesc(nbits=nbits, dim=dim, n_centroids=C, centroids=_addr(keep[0]), bucket_weights=_addr(keep[1]),
                            n_docs_total=total, doc_begin=begin, doc_end=end, doc_len=doc_len, variable_len=0, seed=1)
    d._keep = keep
    return d


def _create(L, desc, entry="fp_index_create"):
    """-> (return code, *out afterwards)"""
    out = ctypes.c_void_p(SENTINEL)
    rc = getattr(L, entry)(ctypes.byref(desc), 0, ctypes.byref(out))
    return rc, out.value


def _create_synth(L, desc):
    return _create(L, desc, "fp_index_create_synthetic")


# (id, creator, descriptor, return code, fp_last_error())
CREATE_CASES = [
    ("create-nbits-3", _create, lambda: _desc(nbits=3), FP_EINVAL, NBITS),
    ("create-dim-4", _create, lambda: _desc(dim=4), FP_EUNSUPPORTED, DIM),
    ("create-dim-12", _create, lambda: _desc(dim=12), FP_EUNSUPPORTED, DIM),
    ("create-dim-1032", _create, lambda: _desc(dim=1032), FP_EUNSUPPORTED, DIM),
    ("create-no-centroids", _create, lambda: _desc(centroids=True), FP_EINVAL, "centroids / bucket_weights missing"),
    ("create-zero-centroids", _create, lambda: _desc(C=0), FP_EINVAL, "centroids / bucket_weights missing"),
    ("create-no-bucket-weights", _create, lambda: _desc(bucket_weights=True), FP_EINVAL, "centroids / bucket_weights missing"),
    ("create-no-doc-lengths", _create, lambda: _desc(doc_lengths=True), FP_EINVAL, "document arrays missing"),
    ("create-no-doc-codes", _create, lambda: _desc(doc_codes=True), FP_EINVAL, "document arrays missing"),
    ("create-no-doc-residuals", _create, lambda: _desc(doc_residuals=True), FP_EINVAL, "document arrays missing"),
    ("create-negative-n-docs", _create, lambda: _desc(n_docs=-1), FP_EINVAL, "document arrays missing"),
    ("create-2^31-1-docs", _create, lambda: _desc(n_docs=2**31 - 1), FP_EUNSUPPORTED, "more than 2^31-1 documents per index shard"),
    ("synthetic-nbits-3", _create_synth, lambda: _synth(nbits=3), FP_EINVAL, NBITS),
    ("synthetic-dim-4", _create_synth, lambda: _synth(dim=4), FP_EUNSUPPORTED, DIM),
    ("synthetic-dim-12", _create_synth, lambda: _synth(dim=12), FP_EUNSUPPORTED, DIM),
    ("synthetic-dim-1032", _create_synth, lambda: _synth(dim=1032), FP_EUNSUPPORTED, DIM),
    ("synthetic-1-centroid", _create_synth, lambda: _synth(C=1), FP_EINVAL, "n_centroids must be a power of two"),
    ("synthetic-48-centroids", _create_synth, lambda: _synth(C=48), FP_EINVAL, "n_centroids must be a power of two"),
    ("synthetic-reversed-range", _create_synth, lambda: _synth(begin=3, end=2), FP_EINVAL, "bad document range"),
    ("synthetic-range-past-the-corpus", _create_synth, lambda: _synth(end=5), FP_EINVAL, "bad document range"),
    ("synthetic-doc-len-0", _create_synth, lambda: _synth(doc_len=0), FP_EINVAL, "doc_len < 1"),
]


@pytest.fixture(scope="module")
def L():
    from fast_plaid_amd import _native
    return _native.lib()


@pytest.mark.parametrize("creator,desc,code,message", [c[1:] for c in CREATE_CASES], ids=[c[0] for c in CREATE_CASES])
def test_creation_refused_before_the_device(L, creator, desc, code, message):
    from fast_plaid_amd import _native
    rc, out = creator(L, desc())
    assert rc == code
    assert _native.last_error() == message
    assert out is None   # (ctypes: a null void* reads as None)


@pytest.mark.parametrize("entry", ["fp_index_create", "fp_index_create_synthetic"])
def test_creation_refuses_null_descriptor_and_null_out(L, entry):
    """a null descriptor is refused before *out is written, so *out starts out null here"""
    from fast_plaid_amd import _native
    out = ctypes.c_void_p()
    assert getattr(L, entry)(None, 0, ctypes.byref(out)) == FP_EINVAL
    assert _native.last_error() == "null argument"
    assert out.value is None
    desc = _desc() if entry == "fp_index_create" else _synth()
    assert getattr(L, entry)(ctypes.byref(desc), 0, None) == FP_EINVAL
    assert _native.last_error() == "null argument"


def test_read_back_of_a_null_index(L):
    from fast_plaid_amd import _native
    buf = np.zeros(64, np.int64)
    assert L.fp_index_read_doc(None, 0, _addr(buf), _addr(buf), 4) == FP_EINVAL
    assert _native.last_error() == "bad document id"
    assert L.fp_index_read_ivf(None, 0, _addr(buf), 4) == FP_EINVAL
    assert _native.last_error() == "bad cell"
    assert L.fp_index_export(None, _addr(buf), _addr(buf), _addr(buf), _addr(buf), _addr(buf)) == FP_EINVAL
    assert _native.last_error() == "null argument"
    assert L.fp_index_ivf_total(None) == 0
    for name in GETTERS:
        assert getattr(L, name)(None) == 0, name
    L.fp_index_destroy(None)   # a no-op


def test_valid_creation_without_a_device_fails_with_a_hip_error(L):
    """only where no device is visible: an otherwise valid creation stops at the device selection and leaves *out null"""
    from fast_plaid_amd import _native
    if L.fp_device_count() == 0:
        for creator, desc in ((_create, _desc()), (_create_synth, _synth())):
            rc, out = creator(L, desc)
            assert rc == FP_EHIP
            assert _native.last_error().startswith("HIP error: ")
            assert out is None
