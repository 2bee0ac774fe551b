"""linprog_batch / libyalps_lpdense.so without a GPU: the numpy restatements of lp_dense_kernel's fill and after against
tableau_model and solution(), the C ABI's header against its binding and the built library, the host-only argument checks of
the library and of the Python call, and the build gate on the new kernels."""
import math
import os
import re

import numpy as np
import pytest

from tests import _np_dense as ND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1, 0), (1, 0, 1), (0, 1, 0), (3, 0, 0), (5, 4, 3), (8, 3, 0), (9, 0, 4))  # (n, m_ub, m_eq)


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpdense()
    return _native


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def random_lp(rng, n, m_ub, m_eq, zeros=True):
    """Operands with zero coefficients of both signs among them (zeros), in c, both matrices and both right-hand sides."""
    def values(*shape):
        a = rng.integers(-4, 9, shape).astype(np.float64) * 0.5
        if zeros and a.size:
            flat = a.reshape(-1)
            flat[rng.integers(0, flat.size, max(1, flat.size // 3))] = 0.0
            flat[rng.integers(0, flat.size, max(1, flat.size // 6))] = -0.0
            flat[0] = 0.0
        return a
    return (values(n), values(m_ub, n) if m_ub else None, values(m_ub) if m_ub else None,
            values(m_eq, n) if m_eq else None, values(m_eq) if m_eq else None)


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
def test_dense_tableau_is_tableau_model_of_the_equivalent_model(shape, maximize):
    from yalps_amd.model import tableau_model
    n, m_ub, m_eq = shape
    for seed in range(4):
        lp = random_lp(np.random.default_rng([7, n, m_ub, m_eq, seed]), *shape)
        t = tableau_model(ND.equivalent_model(*lp, maximize=maximize)).tableau
        m = ND.dense_tableau(*lp, maximize=maximize)
        assert (t.width, t.height) == (n + 1, 1 + m_ub + 2 * m_eq)
        assert np.array_equal(words(m), words(t.matrix)), (shape, maximize, seed)
        # what the comparison is there for: the first entry of every operand is +0.0, which a minimised objective and the
        # second row of an equality turn into -0.0
        minus_zero = (words(m) == np.int64(-2 ** 63)).reshape(t.height, t.width)
        assert n == 0 or minus_zero[0, 1] == (not maximize)
        assert m_eq == 0 or (minus_zero[2 + m_ub, 0] and not minus_zero[1 + m_ub, 0] and (n == 0 or minus_zero[2 + m_ub, 1]))


def test_from_tableau_round_trip(oracle):
    m = oracle.dense_lp(5, 4, 3)
    c, A, b = ND.from_tableau(m, 5, 6)
    assert np.array_equal(words(ND.dense_tableau(c, A, b, maximize=True)), words(m))


def solved(oracle, lp, maximize, **opts):
    n, m_ub, m_eq = ND.shape_of(*lp)
    w, h = n + 1, 1 + m_ub + 2 * m_eq
    m = ND.dense_tableau(*lp, maximize=maximize)
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    status, result, _, _ = oracle.simplex(m, w, h, pos, var, **opts)
    return status, result, m.reshape(h, w)[:, 0].copy(), pos, var


def endings(oracle):
    """[(wanted ending, lp, maximize, options)]: the oracle must produce each (asserted by the test)."""
    A = np.array
    out = [
        ("optimal", (A([3.0, 2.0, 0.0]), A([[1.0, 1.0, 1.0], [1.0, 0.0, 0.0]]), A([4.0, 2.5]), A([[0.0, 1.0, -1.0]]), A([1.0])), True, {}),
        ("optimal", (A([1.0, 2.0]), A([[-1.0, -1.0]]), A([-1.0]), None, None), False, {}),
        ("infeasible", (A([1.0]), A([[1.0]]), A([-1.0]), None, None), True, {}),
        ("cycled", (A([3.0, 2.0, 1.0]), A([[1.0, 1.0, 1.0], [1.0, 0.0, 2.0], [0.0, 1.0, 0.5]]), A([4.0, 2.0, 3.0]), None, None), True,
         {"max_pivots": 1.0}),
        ("unbounded inside", (A([1.0, 1.0]), A([[1.0, -1.0]]), A([2.0]), None, None), True, {}),
    ]
    # unbounded with a slack in the entering column: searched for, the first seed that ends so
    for seed in range(400):
        rng = np.random.default_rng([11, seed])
        lp = (rng.integers(-2, 4, 3).astype(np.float64), rng.integers(-3, 3, (3, 3)).astype(np.float64),
              rng.integers(-2, 5, 3).astype(np.float64), None, None)
        status, result, _, _, var = solved(oracle, lp, True)
        if status == "unbounded" and not 0 <= int(var[int(result)]) - 1 < 3:
            out.append(("unbounded outside", lp, True, {}))
            break
    return out


def test_dense_solution_is_solution(oracle):
    from yalps_amd.model import Tableau, TableauModel
    from yalps_amd.solve import solution
    seen = set()
    for want, lp, maximize, opts in endings(oracle):
        n = len(lp[0])
        status, result, col0, pos, var = solved(oracle, lp, maximize, **opts)
        sign = 1.0 if maximize else -1.0
        if status == "unbounded":
            inside = 0 <= int(var[int(result)]) - 1 < n
            assert want == "unbounded " + ("inside" if inside else "outside"), (want, status, result)
        else:
            assert status == want, (want, status)
        seen.add(want)
        for precision in (1e-8, 0.25):
            x, objective = ND.dense_solution(col0, pos, var, status, result, sign, precision, n)
            tm = TableauModel(Tableau(None, n + 1, col0.size, pos, var, col0), sign, [("x%d" % j, {}) for j in range(n)], [])
            sol = solution(tm, status, result, {"precision": precision, "includeZeroVariables": True})
            rstatus, rx, robjective = ND.model_solution(sol, n)
            assert rstatus == status
            assert np.array_equal(words(np.nan_to_num(x, nan=-7.0)), words(np.nan_to_num(rx, nan=-7.0))), (want, x, rx)
            assert words([objective])[0] == words([robjective])[0] or (math.isnan(objective) and math.isnan(robjective)), (want, objective, robjective)
    assert seen == {"optimal", "infeasible", "cycled", "unbounded inside", "unbounded outside"}, seen


def test_header_symbols_are_exported(nat):
    text = open(os.path.join(ROOT, "include", "yalps_lpdense.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text))
    assert declared, "no declarations parsed"
    L = nat.lpdense_lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(nat.SYMBOLS_LPDENSE)
    others = set(nat.SYMBOLS) | set(nat.SYMBOLS_LPBATCH) | set(nat.SYMBOLS_MILPBATCH) | set(nat.SYMBOLS_LPVAR) | set(nat.SYMBOLS_LPSENS)
    assert not set(nat.SYMBOLS_LPDENSE) & others
    assert "#define YALPS_LPDENSE_MAX_BYTES (4 << 20)" in open(os.path.join(ROOT, "include", "yalps_lpdense.h")).read()
    assert nat.LPDENSE_MAX_BYTES == 4 << 20


FAKE = 4096  # a pointer value validate never dereferences


@pytest.mark.parametrize("args,reason", [
    ((-1, 1, 1, 0, [(FAKE, 0, 1, 0), (FAKE, 0, 1, 1), (FAKE, 0, 1, 0), None, None]), "count < 0"),
    ((1, -1, 1, 0, [None] * 5), "at least 0"),
    ((1, 1, -1, 0, [None] * 5), "at least 0"),
    ((1, 511, 1024, 0, [(FAKE, 0, 1, 0), (FAKE, 0, 511, 1), (FAKE, 0, 1, 0), None, None]), "above the limit"),
    ((1, 511, 0, 512, [(FAKE, 0, 1, 0), None, None, (FAKE, 0, 511, 1), (FAKE, 0, 1, 0)]), "above the limit"),
    ((2, 3, 2, 0, [None, (FAKE, 6, 3, 1), (FAKE, 2, 1, 0), None, None]), "c is NULL"),
    ((2, 3, 2, 0, [(FAKE, 3, 1, 0), None, (FAKE, 2, 1, 0), None, None]), "A_ub is NULL"),
    ((2, 3, 2, 0, [(FAKE, 3, 1, 0), (FAKE, 6, 3, 1), None, None, None]), "b_ub is NULL"),
    ((2, 3, 0, 2, [(FAKE, 3, 1, 0), None, None, None, (FAKE, 2, 1, 0)]), "A_eq is NULL"),
    ((2, 3, 0, 2, [(FAKE, 3, 1, 0), None, None, (FAKE, 6, 3, 1), None]), "b_eq is NULL"),
    ((2, 3, 2, 0, [(FAKE, 3, 1, 0), (FAKE, 6, -3, 1), (FAKE, 2, 1, 0), None, None]), "A_ub: negative stride"),
    ((2, 3, 2, 0, [(FAKE, -3, 1, 0), (FAKE, 6, 3, 1), (FAKE, 2, 1, 0), None, None]), "c: negative stride"),
])
def test_validate_refuses(nat, args, reason):
    with pytest.raises(nat.NativeError, match=re.escape(reason)):
        nat.lpdense_validate(*args)


def test_validate_accepts(nat):
    ok = [(FAKE, 0, 1, 0), (FAKE, 0, 511, 1), (FAKE, 0, 1, 0), None, None]
    nat.lpdense_validate(1, 511, 1023, 0, ok)  # 4 MiB exactly
    nat.lpdense_validate(0, 3, 2, 1, [None] * 5)  # nothing to read
    nat.lpdense_validate(5, 0, 0, 0, [None] * 5)  # w = h = 1
    nat.lpdense_validate(5, 0, 2, 0, [None, None, (FAKE, 0, 1, 0), None, None])  # n = 0: A_ub has no element
    nat.lpdense_validate(5, 2, 0, 1, [(FAKE, 0, 0, 0), None, None, (FAKE, 0, 1, 2), (FAKE, 1, 0, 0)])  # any stride >= 0
    L = nat.lpdense_lib()
    assert L.yalps_lpdense_validate(1, 1, 1, 0, None, None, None, None, None) == -1
    assert b"descriptor is NULL" in L.yalps_lpdense_last_error()


def test_linprog_batch_refuses_before_the_library(nat, monkeypatch):
    import torch
    from yalps_amd import tensors
    monkeypatch.setattr(nat, "LpDense", lambda *a, **k: pytest.fail("the library was touched"))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    L = tensors.linprog_batch
    with pytest.raises(ValueError, match="CPU tensor"):
        L(z(3), z(2, 3), z(2))
    with pytest.raises(ValueError, match="CPU tensor"):
        L(z(4, 3), A_eq=z(2, 3), b_eq=z(4, 2))
    with pytest.raises(TypeError, match="float32"):
        L(z(3).float(), z(2, 3), z(2))
    with pytest.raises(TypeError, match="float32"):
        L(z(3), z(2, 3), z(2).float())
    with pytest.raises(TypeError, match="torch.Tensor"):
        L(np.zeros(3), z(2, 3), z(2))
    with pytest.raises(ValueError, match="4 columns"):
        L(z(3), z(2, 4), z(2))
    with pytest.raises(ValueError, match="2 rows"):
        L(z(3), z(2, 3), z(3))
    with pytest.raises(ValueError, match="disagree about B"):
        L(z(5, 3), z(4, 2, 3), z(2))
    with pytest.raises(ValueError, match="disagree about B"):
        L(z(3), z(4, 2, 3), z(2), z(1, 3), z(5, 1))
    with pytest.raises(ValueError, match="come together"):
        L(z(3), z(2, 3))
    with pytest.raises(ValueError, match="dimensions"):
        L(z(2, 2, 3), z(2, 3), z(2))
    with pytest.raises(ValueError, match=r"solve\(\)"):
        L(z(511), z(1024, 511), z(1024))  # a 1025 x 512 tableau
    with pytest.raises(ValueError, match=r"solve\(\)"):
        L(z(511), A_eq=z(512, 511), b_eq=z(512))
    with pytest.raises(ValueError, match="CPU tensor"):
        L(z(511), z(1023, 511), z(1023))  # 4 MiB exactly passes the size check
    assert tensors.status_names([0, 1, 2, 3]) == ["optimal", "infeasible", "unbounded", "cycled"]


def test_import_yalps_amd_stays_torch_free():
    import subprocess
    import sys
    code = "import sys, yalps_amd, yalps_amd._native; assert 'torch' not in sys.modules, 'torch was imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=120)


def test_kernel_register_budgets(nat):
    """check_register_budgets on the new library: no scratch, no accumulator registers, static LDS a multiple of 16 -- and the
    six forms of the class table are what the code object holds."""
    from yalps_amd import build
    ks = build.check_register_budgets(build.LIB_LPDENSE, min_resident=0)
    dense = [k for k in ks if "lp_dense_kernel" in k]
    assert len(dense) == 6 and len(ks) == 6, sorted(ks)
    for k in dense:
        md = ks[k]
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0 and int(md["group_segment_fixed_size"]) % 16 == 0, (k, md)
    assert "lp_dense" in build.NO_SCRATCH
