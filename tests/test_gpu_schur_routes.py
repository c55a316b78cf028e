"""GPU parity of the Schur driver's routes run IN A ROW on one workspace and one factor image (spasm_hip_dschur).

Every other test gives each route a fresh workspace.  Here the routes follow each other, so that whatever one call leaves
behind meets the next: the accumulator scratch under its all-zero invariant (32-bit and 64-bit layouts in one buffer),
buffers grown by one route and reused by another, the row lengths and look-back words of the previous call, events recorded
by one route and read by the statistics of another.  Every call is compared with the oracle's Schur complement of the same
rows, bit for bit (oracle.same_matrix), and with what the statistics must say about the route it took.

The library reads the environment at every look-up: setting a switch between two calls switches the route."""
import numpy as np
import pytest

import spasm_amd

pytestmark = pytest.mark.gpu

SWITCHES = ("SPASM_HIP_BACKSOLVE", "SPASM_HIP_GROUP", "SPASM_HIP_FORCE_TIER", "SPASM_HIP_BS_DIRECT", "SPASM_HIP_SPARSE_IMAGE")


def _as_product(A):
    return spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, A.prime)


def _fact(F):
    return spasm_amd.Fact(_as_product(F.U), F.qinv)


class _Problem:
    """A, its structural pivots, the rows to reduce, the oracle's S (computed once, never changed), and the device images"""

    def __init__(self, oracle, p, n, m, ti, tj, tx):
        import torch
        self.p = p
        self.A = oracle.compress(p, n, m, ti, tj, tx)
        npiv, perm, F = oracle.pivots_extract_structural(self.A, oracle.empty_fact(self.A.n, self.A.m, p))
        self.rows = perm[npiv:]
        self.want, _, _ = oracle.schur(self.A, self.rows, F)
        self.dA = spasm_amd.DeviceCsr.from_host(_as_product(self.A))
        self.dF = spasm_amd.DeviceFact(_fact(F))
        self.drows = torch.from_numpy(np.ascontiguousarray(self.rows, np.int32)).cuda()
        self.nnz = set()


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("SPASM_HIP_" + k, v)


def _call(oracle, monkeypatch, P, W, label, env, problems):
    """one call under `env`: S against the oracle, and the checks every call must pass.  Returns the statistics."""
    _set(monkeypatch, env)
    S, st = spasm_amd.dschur(P.dA, P.drows, P.dF, W)
    where = "%s at p = %d" % (label, P.p)
    print(where, {f: getattr(st, f) for f, _ in st._fields_ if not f.startswith("ms_")})
    assert st.status == 0 and S is not None, where
    H = S.to_host()
    if not oracle.same_matrix(oracle.CSR(H.n, H.m, H.p, H.j, H.x, P.p), P.want):
        problems.append(where + ": S differs from the oracle's")
    P.nnz.add(int(st.nnz))
    if st.rows != len(P.rows):
        problems.append(where + ": rows")
    if not st.kernel:
        problems.append(where + ": no kernel name")
    built = bool(st.backsolve_built or st.sparse_image_built)
    # kernel_other: named when this call built R, empty on a row route.  (An image route that found R in place names the build
    # kernel there all the same, so "empty when nothing was built" is not asked of those calls: DESIGN.md section 8.)
    if built and not st.kernel_other:
        problems.append(where + ": R was built and kernel_other is empty")
    if not (st.used_backsolve or st.used_sparse_image) and st.kernel_other:
        problems.append(where + ": kernel_other = %r on a row route" % st.kernel_other)
    return st


def _expect(problems, where, st, **fields):
    for f, v in fields.items():
        if getattr(st, f) != v:
            problems.append("%s: %s = %r, expected %r" % (where, f, getattr(st, f), v))


def _row_routes(problems, where, st):
    _expect(problems, where, st, used_backsolve=0, used_sparse_image=0)
    if st.rows_lds + st.rows_lds_big + st.rows_dense != st.rows:
        problems.append("%s: tiers %d + %d + %d of %d rows" % (where, st.rows_lds, st.rows_lds_big, st.rows_dense, st.rows))


def test_routes_in_a_row_on_a_narrow_factor(oracle, monkeypatch):
    """3000 x 2000, three entries a row (test_schur_random_fill_in), p = 42013 and 4294967291 (64-bit sums: another scratch
    layout in the same buffer).  One factor image per prime, made under the default environment (it has the plan of the dense
    image); one workspace for both."""
    _set(monkeypatch, {})
    n, m, per_row = 3000, 2000, 3
    prob = {}
    for p in (42013, 4294967291):
        rng = np.random.default_rng(n + m)
        ti = np.repeat(np.arange(n, dtype=np.int32), per_row)
        tj = rng.integers(0, m, size=n * per_row).astype(np.int32)
        tx = rng.integers(1, p, size=n * per_row).astype(np.int64)
        prob[p] = _Problem(oracle, p, n, m, ti, tj, tx)
    W = spasm_amd.SchurWorkspace(max(len(P.rows) for P in prob.values()), m, 4 * max(P.want.nnz for P in prob.values()) + (1 << 22))
    problems = []
    P = prob[42013]
    nrows = len(P.rows)

    def call(label, env, P=P):
        return _call(oracle, monkeypatch, P, W, label, env, problems)

    _row_routes(problems, "(i)", call("(i)", {"BACKSOLVE": "0"}))
    _expect(problems, "(ii)", call("(ii)", {"BACKSOLVE": "0", "GROUP": "1"}), used_group_kernel=1, group_aborted=0)
    _expect(problems, "(iii)", call("(iii)", {"BACKSOLVE": "0", "FORCE_TIER": "2"}), rows_dense=nrows)
    _expect(problems, "(iv)", call("(iv)", {"BACKSOLVE": "0", "FORCE_TIER": "1"}), rows_lds=0)
    _expect(problems, "(v)", call("(v)", {"BACKSOLVE": "1"}), used_backsolve=1, backsolve_built=1)
    _expect(problems, "(vi)", call("(vi)", {"BACKSOLVE": "1", "BS_DIRECT": "0"}), used_backsolve=1, backsolve_built=0)
    _expect(problems, "(vii)", call("(vii)", {}), used_backsolve=1)          # (R is there)
    _row_routes(problems, "(viii)", call("(viii)", {"BACKSOLVE": "0"}))
    Q = prob[4294967291]
    _expect(problems, "(ii) wide", call("(ii)", {"BACKSOLVE": "0", "GROUP": "1"}, Q), used_group_kernel=1, group_aborted=0)
    _expect(problems, "(iii) wide", call("(iii)", {"BACKSOLVE": "0", "FORCE_TIER": "2"}, Q), rows_dense=len(Q.rows))
    _expect(problems, "(v) wide", call("(v)", {"BACKSOLVE": "1"}, Q), used_backsolve=1, backsolve_built=1)
    _expect(problems, "(iii) again", call("(iii) again", {"BACKSOLVE": "0", "FORCE_TIER": "2"}), rows_dense=nrows)
    for R in prob.values():
        if len(R.nnz) != 1:
            problems.append("p = %d: nnz differs between the calls: %s" % (R.p, sorted(R.nnz)))
    W.close()
    for R in prob.values():
        R.dF.close()
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("nnon", [1, 8193])
def test_the_sparse_image_between_row_routes(oracle, monkeypatch, nnon):
    """the smallest system of test_gpu_sparse_image.py (test_sparse_image_column_counts: 500 pivots, 300 rows, one
    non-pivotal column) and the one just over a segment of 8,192 columns: sparse image (built), row routes, sparse image
    again (R is there) on one workspace."""
    from test_gpu_sparse_image import _triangular_system
    p = 42013
    _set(monkeypatch, {"SPARSE_IMAGE": "1"})          # (at the factor's creation: it gets the plan of the sparse image)
    rng = np.random.default_rng(nnon)
    P = _Problem(oracle, p, *_triangular_system(rng, p, npiv=500, nnon=nnon, nred=300, deps=lambda k: 2, reach=40, np_per_row=3, red_entries=5))
    W = spasm_amd.SchurWorkspace(len(P.rows), P.A.m, 4 * P.want.nnz + (1 << 22))
    problems = []
    sts = [("first", _call(oracle, monkeypatch, P, W, "first", {"SPARSE_IMAGE": "1"}, problems)),
           ("second", _call(oracle, monkeypatch, P, W, "second", {"SPARSE_IMAGE": "0", "BACKSOLVE": "0"}, problems)),
           ("third", _call(oracle, monkeypatch, P, W, "third", {"SPARSE_IMAGE": "1"}, problems))]
    _expect(problems, "first", sts[0][1], used_sparse_image=1, sparse_image_built=1)
    _row_routes(problems, "second", sts[1][1])
    _expect(problems, "third", sts[2][1], used_sparse_image=1, sparse_image_built=0)
    for where, st in sts:
        if (st.ms_sparse_build == 0) != (st.sparse_image_built == 0):
            problems.append("%s: ms_sparse_build = %g with sparse_image_built = %d" % (where, st.ms_sparse_build, st.sparse_image_built))
    if len(P.nnz) != 1:
        problems.append("nnz differs between the calls: %s" % sorted(P.nnz))
    W.close()
    P.dF.close()
    assert not problems, "\n".join(problems)
