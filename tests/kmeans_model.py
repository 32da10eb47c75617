"""numpy restatement of fp_kmeans (include/fastplaid.h states the arithmetic; this file restates exactly that and nothing of the
product's code -- the product must not import it):

  1. cent32[c] = (float)data[init_rows[c]]
  for it in range(niter):
  2. cent16 = RNE16(cent32); hn[c] = 0.5f * ascending-d fp32 chain of cent16[c][d]^2
  3. label[t] = argmax_c fl32(chain(t, c) - hn[c]), chain = ascending-d fp32 sum of data[t][d] * cent16[c][d], ties -> lowest c
  4. S[c][d] = exact sum of data[t][d] over label[t] == c as int64 in units of 2^-24, cnt[c] the count
  5. cnt[c] > 0:  cent32[c][d] = (float)(((double)S * 2^-24) / (double)cnt[c])
  6. cnt[c] == 0: cent32[c] = (float)data[rnd(seed, 0x6B6D0000 + it, c) % n]
"""
import numpy as np

from fast_plaid_amd import synth

RESEED_STREAM = 0x6B6D0000


def fixed(x16: np.ndarray) -> np.ndarray:
    """finite fp16 values as int64 multiples of 2^-24 (exact: the smallest subnormal is 2^-24, the product fits a double)"""
    return (np.asarray(x16, np.float16).astype(np.float64) * 2.0 ** 24).astype(np.int64)


def refused(n: int, max_abs16) -> bool:
    """the header's bound: the call is refused when n * max|x| * 2^24 >= 2^62"""
    return int(n) * abs(int(fixed(np.float16(max_abs16)))) >= 2 ** 62


def prepare(cent32: np.ndarray):
    """step 2 -> (cent16, hn)"""
    cent16 = cent32.astype(np.float16)
    c = cent16.astype(np.float32)
    acc = np.zeros(c.shape[0], np.float32)
    for d in range(c.shape[1]):
        acc = acc + c[:, d] * c[:, d]      # fp32: the square of an fp16 value is exact, the addition rounds once
    return cent16, (np.float32(0.5) * acc).astype(np.float32)


def assign(data16: np.ndarray, cent16: np.ndarray, hn: np.ndarray) -> np.ndarray:
    """step 3"""
    x = data16.astype(np.float32)
    c = cent16.astype(np.float32)
    acc = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for d in range(x.shape[1]):
        acc += x[:, d, None] * c[None, :, d]
    return np.argmax(acc - hn[None, :], axis=1).astype(np.int64)   # first maximal value = lowest index


def sums(data16: np.ndarray, labels: np.ndarray, k: int):
    """step 4 -> (S int64 [k, dim], cnt int64 [k])"""
    S = np.zeros((k, data16.shape[1]), np.int64)
    np.add.at(S, labels, fixed(data16))
    return S, np.bincount(labels, minlength=k).astype(np.int64)


def run(data16: np.ndarray, k: int, niter: int, init_rows: np.ndarray, seed: int):
    """-> dict: cent32 / counts after every iteration count 0 .. niter (lists indexed by the number of iterations run),
    labels and cent16 of every iteration, the number of reseeded clusters per iteration"""
    data16 = np.ascontiguousarray(data16, np.float16)
    n = data16.shape[0]
    cent32 = data16[np.asarray(init_rows)].astype(np.float32)
    out = dict(cent32=[cent32.copy()], counts=[np.zeros(k, np.int64)], labels=[], cent16=[], hn=[], reseeds=[])
    for it in range(niter):
        cent16, hn = prepare(cent32)
        labels = assign(data16, cent16, hn)
        S, cnt = sums(data16, labels, k)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = ((S.astype(np.float64) * 2.0 ** -24) / cnt[:, None].astype(np.float64)).astype(np.float32)
        empty = np.flatnonzero(cnt == 0)
        r = (synth.rnd(seed, RESEED_STREAM + it, empty) % np.uint64(n)).astype(np.int64)
        cent32 = mean
        cent32[empty] = data16[r].astype(np.float32)
        out["cent32"].append(cent32.copy())
        out["counts"].append(cnt)
        out["labels"].append(labels)
        out["cent16"].append(cent16)
        out["hn"].append(hn)
        out["reseeds"].append(int(empty.size))
    return out
