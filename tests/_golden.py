"""Decoders for tests/golden/*.json.gz (data emitted by oracle/tools/gen_golden.py)."""
import base64
import functools
import gzip
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dec(s, dtype):
    return np.frombuffer(base64.b64decode(s), dtype=dtype).copy()


def _num(x):
    return float(x) if isinstance(x, str) else x


@functools.lru_cache(None)
def records(kind):
    with gzip.open(os.path.join(GOLDEN, f"simplex_{kind}.json.gz")) as f:
        return json.load(f)["records"]


def label(rec):
    if rec["kind"] == "case":
        return rec["name"]
    return "%s-%dx%d-s%d" % (rec["kind"], rec["M"], rec["N"], rec["seed"])


def sha256(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


NAN_WORD = 0x7FF8000000000000


def canon(arr):
    """A copy with every NaN word replaced by the quiet NaN 0x7ff8000000000000: all NaNs are one value."""
    out = np.ascontiguousarray(arr, dtype=np.float64).copy()
    out.view(np.uint64)[np.isnan(out)] = NAN_WORD
    return out


def sha256_canon(arr):
    """SHA-256 of the doubles with all NaNs made one value (the reference's engine and a GPU give arithmetic NaNs different
    sign bits and payloads)."""
    return sha256(canon(arr))


def initial_matrix(rec, oracle=None, dense_gen=None):
    """Initial row-major tableau of a record (COO-decoded, or regenerated for dense records)."""
    w, h = rec["width"], rec["height"]
    if "init_coo" in rec:
        m = np.zeros(w * h, np.float64)
        m[_dec(rec["init_coo"]["idx"], np.int32)] = _dec(rec["init_coo"]["val"], np.float64)
    else:
        gen = dense_gen if dense_gen is not None else oracle.dense_lp
        m = gen(rec["M"], rec["N"], rec["seed"])
    assert sha256(m) == rec["init_sha256"], "initial tableau differs from the reference's"
    return m


def _perm(x):
    """A permutation: base64 int32, or (edge records) {"n", "idx", "val"}: the entries that differ from the identity."""
    if isinstance(x, str):
        return _dec(x, np.int32)
    p = np.arange(x["n"], dtype=np.int32)
    p[_dec(x["idx"], np.int32)] = _dec(x["val"], np.int32)
    return p


def expected(rec):
    """col0 is None where a record keeps only its digest (col0_sha256: edge records of more than 1024 rows).  The
    non-finite records (tests/_nonfinite.py) hold col0 and the digests with all NaNs made one value (`*_canon_sha256`)."""
    return dict(status=rec["status"], result=_num(rec["result"]), n_pivots=rec["n_pivots"],
                pivots=_dec(rec["pivots"], np.int32).reshape(-1, 2), pos=_perm(rec["pos"]), var=_perm(rec["var"]),
                col0=_dec(rec["col0"], np.float64) if "col0" in rec else None, col0_sha256=rec.get("col0_sha256"),
                final_sha256=rec.get("final_sha256"), col0_canon_sha256=rec.get("col0_canon_sha256"),
                final_canon_sha256=rec.get("final_canon_sha256"))


def options(rec):
    o = rec["options"]
    return dict(precision=_num(o["precision"]), max_pivots=_num(o["maxPivots"]), check_cycles=o["checkCycles"])


def identity_perms(rec):
    n = rec["width"] + rec["height"]
    return np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)


def same_number(a, b):
    """Equal as numbers: -0.0 and +0.0 are the same here.  The golden files written before simplex_rounding.json.gz hold
    `result` as a JSON number, and JSON.stringify(-0) is "0": they cannot say which zero the reference produced, so a
    comparison with them cannot ask for one.  The sign of a rounded zero is pinned by tests/golden/simplex_rounding.json.gz
    and simplex_rounding_edges.json.gz (tests/_rounding.py), whose floats are 64-bit words in hex: compare with same_bits."""
    return (a != a and b != b) or a == b


def same_bits(a, b):
    """Equal word for word, all NaNs one value: tells -0.0 from +0.0."""
    return canon(np.array([a], np.float64)).tobytes() == canon(np.array([b], np.float64)).tobytes()
