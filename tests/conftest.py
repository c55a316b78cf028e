import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the tests pick kernel variants and debugging aids by name: switches outside the supported list need this (spasm_hip.h, "Environment")
os.environ.setdefault("SPASM_HIP_EXPERIMENT", "1")

GOLDEN = os.path.join(ROOT, "tests", "golden")

# moduli and matrices of the reference's own suite (tests/CMakeLists.txt:45-52, 75-110)
ALL_MODULI = [3, 257, 65537, 67108859, 189812507, 4294967291]
ALL_TEST_MATRICES = [
    "BIOMD0000000424.int.mpl.sms", "cc.sms", "chains.sms", "dm.sms", "example.sms", "G2.sms",
    "lower_trapeze.sms", "mat364.sms", "p3.sms", "rectangular_l.sms", "scc3.sms", "singular2.sms",
    "singular.sms", "t1.sms", "upper_trapeze.sms", "BIOMD0000000525.int.mpl.sms", "chains2.sms",
    "dm2.sms", "empty.sms", "g1.sms", "l1.sms", "m1.sms", "medium.sms", "rectangular_h.sms",
    "scc2.sms", "scc.sms", "singular3.sms", "small.sms", "tree_test.sms", "trefethen_500.sms",
    "u1.sms", "void.sms",
]


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def matrix_path(name):
    return os.path.join(GOLDEN, "Matrix", name)


# What the compiled reference (oracle/_ref) returns on the suite's own inputs, stored in tests/golden/reference/<family>.npz
# (one array per "<case>|<field>"), so that the comparisons with the reference also run where its tree was absent at build time.
# Where oracle/_ref was built, every vector is recomputed by the reference and must equal the stored one.  To rewrite them
# (a new case, a new matrix), build with the reference tree present and run the tests that ask for them with
# SPASM_RECORD_REFERENCE=1.
REFERENCE_VECTORS = os.path.join(GOLDEN, "reference")
_stored_vectors = {}
_recorded_vectors = {}


def _stored(family):
    if family not in _stored_vectors:
        import numpy as np
        index = {}
        path = os.path.join(REFERENCE_VECTORS, family + ".npz")
        if os.path.exists(path):
            with np.load(path) as z:
                for name in z.files:
                    case, field = name.rsplit("|", 1)
                    index.setdefault(case, {})[field] = z[name]
        _stored_vectors[family] = index
    return _stored_vectors[family]


def reference_vectors(oracle, family, case, live):
    """the arrays live() computes with the compiled reference for `case` of `family` (a dict of arrays)."""
    import numpy as np
    record = os.environ.get("SPASM_RECORD_REFERENCE") == "1"
    got = None
    if oracle.ref_available():
        got = {k: np.asarray(v) for k, v in live().items()}
        if record:
            _recorded_vectors.setdefault(family, {}).update({"%s|%s" % (case, k): v for k, v in got.items()})
            return got
    elif record:
        pytest.fail("SPASM_RECORD_REFERENCE=1 needs oracle/_ref (built when the reference tree is present)")
    want = _stored(family).get(case)
    assert want is not None, "no stored reference vector %s/%s (record it with SPASM_RECORD_REFERENCE=1)" % (family, case)
    if got is not None:
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in got), \
            "the compiled reference no longer returns the stored vector %s/%s" % (family, case)
    return want


def pytest_sessionfinish(session, exitstatus):
    import numpy as np
    for family, arrays in _recorded_vectors.items():
        path = os.path.join(REFERENCE_VECTORS, family + ".npz")
        merged = {}
        if os.path.exists(path):
            with np.load(path) as z:
                merged = {name: z[name] for name in z.files}
        merged.update(arrays)
        os.makedirs(REFERENCE_VECTORS, exist_ok=True)
        np.savez_compressed(path, **merged)


def csr_arrays(S):
    """a CSR (oracle.CSR or spasm_amd.Csr) as the arrays reference_vectors() stores."""
    return {"n": S.n, "m": S.m, "p": S.p, "j": S.j, "x": S.x}


def csr_of(oracle, d, prime):
    return oracle.CSR(int(d["n"]), int(d["m"]), d["p"], d["j"], d["x"], prime)


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle as orc
    orc.lib()
    return orc
