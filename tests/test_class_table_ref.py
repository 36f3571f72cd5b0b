"""The premises of tests/test_gpu_class_table.py, on the CPU.  The GPU module takes every expected value from the oracle under
scoring systems whose class-table entries can be told apart (tests/class_table.py); here the oracle is pinned to the reference on
those very systems -- live where oracle/_ref is built, through tests/golden/class_table_vectors.npz everywhere -- and every
(system, family) pair of the GPU module is shown to be sensitive: each of nine confusions of the table, and for `distinct` each
change of one of its 36 entries by one, changes what the oracle returns.  Where a confusion cannot show by definition, that is
asserted instead: under `nocase` two of the nine give back the same matrix (lower case folded, N's candidates rotated), so seven
are checked there; the packed library form holds no lower case, so its cases are checked for the two N confusions and shown to
read no lower-case row; the LEAN band's family is on the plus strand only, which its premises say.  The gates are checked with one lone extreme entry in a
lower-case class, in N and in an upper-case class, against the library's own planners."""
import ctypes
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from repeatafterme_amd import _lib

import class_table as ct
import score_gates as sg
from helpers import GOLDEN, assert_same_result

FIXTURE = os.path.join(GOLDEN, "class_table_vectors.npz")


def test_systems_are_what_they_are_said_to_be():
    ct.check_systems()
    for name in ct.SYSTEMS:
        for W in sorted({w for _, w in ct.ALL_GPU_FAMILIES} | set(ct.REF_WIDTHS)):
            for L in (96, ct.REF_L, 1000):
                assert ct.gates(name, W, L) == ct.expected_gates(name, W), (name, W, L, ct.gates(name, W, L))
    m, go, ge = ct.matrix_of("distinct")
    for W in sg.PK_WIDTHS:                                   # the packed rows with thousands to spare, at every width
        assert sg.pk_plan(W, go, ge, m).total <= sg.PK_LIMIT - 10000
    assert len(ct.CONFUSIONS) == 9 and len(ct.single_entry_changes(m)) == 72
    for tag, changed in ct.single_entry_changes(m):
        assert (changed != m).sum() == 1 and abs(int((changed - m).sum())) == 1, tag


# ---- the oracle against the reference -----------------------------------------------------------------------------------------------

def _oracle_case(fs, p):
    c, m = fs.cores.copy(), po.new_master(p.L)
    rr = po.oracle_extend(1, c, fs.sequence, m, p)
    rl = po.oracle_extend(0, c, fs.sequence, m, p)
    return c, m, (rr, rl)


@pytest.mark.skipif(not po.have_ref(), reason="the compiled reference (oracle/_ref) is not built here")
@pytest.mark.parametrize("kind", ["soft", "adversarial"])
@pytest.mark.parametrize("name", ct.SYSTEMS)
def test_oracle_equals_the_reference_live(name, kind):
    """All five systems at W = 0, 1, 7, 14, 40 on six soft-masked families and six adversarial sets, both directions."""
    seen = 0
    for k, seed, W, nm in ct.ref_cases():
        if (k, nm) != (kind, name):
            continue
        fs, p = ct.ref_family(kind, seed, W), ct.system(name, W, ct.REF_L)
        c1, m1 = fs.cores.copy(), po.new_master(p.L)
        r1 = (po.ref_extend(1, c1, fs.sequence, m1, p, boundaries=fs.boundaries), po.ref_extend(0, c1, fs.sequence, m1, p, boundaries=fs.boundaries))
        c2, m2, r2 = _oracle_case(fs, p)
        assert_same_result(c1, m1, r1, c2, m2, r2, f"{kind} seed {seed} W={W} {name}")
        seen += 1
    assert seen == len(ct.REF_SEEDS) * len(ct.REF_WIDTHS)


def test_oracle_equals_the_recorded_reference():
    """The same cases from the fixture (the reference's results as tests/golden/make_class_table_golden.py recorded them): the
    fixture's inputs are those tests/class_table.py builds today, and the oracle gives what the reference gave."""
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(GOLDEN, "api_vectors.npz"))
    z = np.load(FIXTURE)
    assert [str(s) for s in z["systems"]] == list(ct.SYSTEMS)
    for name in ct.SYSTEMS:
        m, go, ge = ct.matrix_of(name)
        assert np.array_equal(z[f"table_{name}"], sg.class_table(m).T) and tuple(z[f"gaps_{name}"]) == (go, ge), name
    cases = ct.ref_cases()
    assert len(z["cases"]) == len(cases) == 300
    fields = ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext", "right_ext", "seq_idx")
    at, kinds_seen = 0, set()
    for row, ret, master, (kind, seed, W, name) in zip(z["cases"], z["ret"], z["master"], cases):
        j = int(row[0])
        assert tuple(row[1:]) == (("soft", "adversarial").index(kind), seed, W, ct.SYSTEMS.index(name))
        fs = ct.ref_family(kind, seed, W)
        assert np.array_equal(z[f"f{j}_sequence"], fs.sequence) and np.array_equal(z[f"f{j}_boundaries"], fs.boundaries)
        assert np.array_equal(z[f"f{j}_cores"], np.array([getattr(fs.cores, f) for f in fields], np.int64))
        p = ct.system(name, W, ct.REF_L)
        assert tuple(z["stop"]) == (p.cappenalty, p.minimprovement, p.L, p.when_to_stop)
        c, m, res = _oracle_case(fs, p)
        tag = f"{kind} seed {seed} W={W} {name}"
        assert (res[0].ret, res[1].ret) == tuple(ret), tag
        assert np.array_equal(m, master), f"{tag}: consensus differs at {np.nonzero(m != master)[0][:8]}"
        want = z["per_copy"][:, at:at + c.n]
        at += c.n
        assert np.array_equal(want, np.array([c.left_len, c.right_len, c.score], np.int32)), tag
        kinds_seen.add((kind, name, W))
    assert at == z["per_copy"].shape[1] and len(kinds_seen) == 2 * 5 * 5


def test_reference_cases_are_not_soft():
    """The pinned cases do extend, through soft-masked bases on both strands and through N; under `distinct` every confusion
    changes the result of at least one of them (the pin would notice an oracle that had the table wrong)."""
    for seed in ct.REF_SEEDS:
        run = ct.Run("distinct", ct.ref_family("soft", seed, 14), ct.system("distinct", 14, ct.REF_L),
                     *ct.run_oracle(ct.ref_family("soft", seed, 14), ct.system("distinct", 14, ct.REF_L)))
        ct.check_family(run)
    runs = []
    for seed in ct.REF_SEEDS:
        for W in ct.REF_WIDTHS:
            fs, p = ct.ref_family("soft", seed, W), ct.system("distinct", W, ct.REF_L)
            runs.append(ct.Run("distinct", fs, p, *ct.run_oracle(fs, p)))
    blind = [what for what, f in ct.CONFUSIONS.items() if not any(ct.differs(run, f(run.p.matrix)) for run in runs)]
    assert not blind, blind


# ---- sensitivity: a condition on the inputs of the GPU module, checked on the oracle alone --------------------------------------------

NO_CHANGE_UNDER_NOCASE = ("lower case folded onto upper case", "N's candidates rotated")


@pytest.mark.parametrize("n,W", ct.ALL_GPU_FAMILIES, ids=[f"{n}x{w}" for n, w in ct.ALL_GPU_FAMILIES])
@pytest.mark.parametrize("name", ["distinct", "nocase"])
def test_every_confusion_changes_the_oracles_result(name, n, W):
    """Each of the nine confusions must change ret, rows, consensus, lengths or scores in at least one direction, for every
    (system, family) pair the GPU module runs.  Two confusions cannot, by the definition of the system: `nocase` holds the upper-case
    block in the lower-case columns and -1 for N under every candidate, so folding lower case onto upper case and rotating N's
    candidates give back the same matrix -- asserted as such; the other seven must show."""
    run = ct.oracle_run(name, n, W)
    ct.check_family(run)
    blind = []
    for what, f in ct.CONFUSIONS.items():
        changed = f(run.p.matrix)
        if name == "nocase" and what in NO_CHANGE_UNDER_NOCASE:
            assert np.array_equal(changed, run.p.matrix)
            continue
        assert not np.array_equal(changed, run.p.matrix), what
        if not ct.differs(run, changed):
            blind.append(what)
    print(f"{name} {n} x W={W}: blind confusions {blind}")
    assert not blind, (name, n, W, blind)


@pytest.mark.parametrize("W,n", ct.SMALLEST_PER_WIDTH, ids=[f"W{w}" for w, _ in ct.SMALLEST_PER_WIDTH])
def test_every_single_entry_changes_the_oracles_result(W, n):
    """`distinct` on the smallest family of each band width: changing any one of the 36 entries by +1 or -1 changes the result."""
    run = ct.oracle_run("distinct", n, W)
    blind = [tag for tag, changed in ct.single_entry_changes(run.p.matrix) if not ct.differs(run, changed)]
    print(f"distinct {n} x W={W}: blind entries {blind}")
    assert not blind, (n, W, blind)


@pytest.mark.parametrize("n,W", ct.ALL_GPU_FAMILIES, ids=[f"{n}x{w}" for n, w in ct.ALL_GPU_FAMILIES])
def test_n_confusions_change_the_result_under_n_pays(n, W):
    run = ct.oracle_run("n_pays", n, W)
    ct.check_family(run)
    blind = [what for what in ct.N_CONFUSIONS if not ct.differs(run, ct.CONFUSIONS[what](run.p.matrix))]
    assert not blind, (n, W, blind)


def test_lean_family_is_sensitive():
    """The LEAN band's family under `distinct` (the pair of test_gpu_class_table.py::test_lean_band): its premises, and each of
    the nine confusions changes the oracle's result."""
    run = ct.lean_run()
    ct.check_lean_family(run)
    assert ct.gates("distinct", ct.LEAN_W, ct.LEAN_L) == ct.expected_gates("distinct", ct.LEAN_W)
    blind = [what for what, f in ct.CONFUSIONS.items() if not ct.differs(run, f(run.p.matrix))]
    assert not blind, blind


@pytest.mark.parametrize("W", [0, 14, 40, 80])
@pytest.mark.parametrize("name", ["distinct", "n_pays"])
def test_packed_library_cases_are_sensitive(name, W):
    """The cases of test_gpu_class_table.py::test_packed_library_form run on the FOLDED library: the packed form carries N but no
    case, so the library holds no lower-case base and the seven lower-case confusions cannot show there -- asserted as such.  The
    two N confusions must, in every case, under both systems; and N runs cross window and word borders of the tables used."""
    import window_cases as wc
    import window_ref as wr
    assert tuple(wc.LOOP_W) == (0, 14, 40, 80)
    cases = wc.loop_cases(W)
    assert ct.gates(name, W, cases[0].L) == ct.expected_gates(name, W)
    for c in cases:
        lib = wr.fold(c.lib)
        assert (lib == 99).any() and not ((lib >= 4) & (lib < 8)).any() and ((c.lib >= 4) & (c.lib < 8)).any(), c.name
        assert ct.n_runs_cross_borders(ct.windows_inside_n_runs(c)) == (True, True), c.name
        p = ct.system(name, W, c.L, when_to_stop=ct.LOOP_WHEN_TO_STOP)
        assert ct.loop_run(name, c)[4].rows_executed > 0
        for what, f in ct.CONFUSIONS.items():
            if what in ct.N_CONFUSIONS:
                assert ct.loop_differs(name, c, f(p.matrix)), (c.name, what)
            else:                                            # (they change lower-case rows of the table only, which nothing here reads)
                assert np.array_equal(sg.class_table(f(p.matrix))[[0, 1, 2, 3, 8]], sg.class_table(p.matrix)[[0, 1, 2, 3, 8]]), what


@pytest.mark.parametrize("n,W", ct.ALL_GPU_FAMILIES, ids=[f"{n}x{w}" for n, w in ct.ALL_GPU_FAMILIES])
def test_control_the_builtin_system_is_blind(n, W):
    """With 14p43g on the same families the classes 4..8 hold one constant: swapping 4<->7 and 5<->6 and reading N as a, all at
    once, gives back the same matrix -- which is why no test on a built-in system could see the table.  The oracle is run on the
    changed matrix for the families of up to 720 copies only: the matrix being the same one, a second run of the larger ones
    would spend half a minute to say that the oracle gives the same result twice."""
    p = ct.system("14p43g", W, 96)
    changed = ct.control(p.matrix)
    assert np.array_equal(changed, p.matrix)
    t = sg.class_table(p.matrix)
    assert len(set(t[4:].reshape(-1).tolist())) == 1
    if n <= 720:
        run = ct.oracle_run("14p43g", n, W)
        assert not ct.differs(run, changed)


# ---- the gates with one lone extreme entry ---------------------------------------------------------------------------------------

def _planners():
    """ramx_pk_plan and ramx_cp_max_family of libramx.so (C++ linkage; the class table goes in by reference, that is as a pointer)."""
    assert os.path.exists(_lib.LIB_PATH), "build libramx.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    # The two planners have C++ linkage: their exported names carry their signatures (Itanium ABI: int, int, int, a reference
    # to const int[9][4], then two int* or an int).  A changed signature changes the name -- and must change the call below.
    names = {"ramx_pk_plan": "_Z12ramx_pk_planiiiRA9_A4_KiPiS3_", "ramx_cp_max_family": "_Z18ramx_cp_max_familyiiiRA9_A4_Kii"}
    for plain, mangled in names.items():
        assert hasattr(lib, mangled), (f"libramx.so does not export {plain}(int, int, int, const int (&)[9][4], ...) as {mangled}: "
                                       f"its signature has changed (csrc/ramx_pk_api.h, csrc/ramx_cp_api.h); adapt this call")
    pk, cp = getattr(lib, names["ramx_pk_plan"]), getattr(lib, names["ramx_cp_max_family"])
    pk.restype = cp.restype = ctypes.c_int
    pk.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    cp.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_int]
    return pk, cp


def test_gates_with_one_lone_extreme_entry(monkeypatch):
    """Exactly one entry at 127, 128, -128 or -129, in a lower-case class, in N, in an upper-case class: the restated gates flip
    with the int8 range wherever the entry sits, P and mn see it, and the library's planners decide as the restatement does."""
    for k in ("RAMX_NO_PK", "RAMX_NO_CP"):
        monkeypatch.delenv(k, raising=False)
    pk, cp = _planners()
    systems = ct.extreme_systems()
    assert len(systems) == 12
    base = ct.matrix_of("distinct")[0]
    for tag, m, go, ge in systems:
        assert (m != base).sum() == 1, tag
        v = int(m[m != base][0])
        int8 = -128 <= v <= 127
        P, mn = sg.p_mn(m)
        assert (P, mn) == ((v, 26) if v > 0 else (12, -v)), (tag, P, mn)
        tab = np.ascontiguousarray(sg.class_table(m), np.int32)
        for W in (14, 40, 80, 9):
            for L in (96, 2000):
                assert sg.fast_pack_ok(W, L, go, ge, m) == int8, (tag, W, L)
                assert sg.cp_value_range_ok(W, L, go, ge, m) == (int8 and W != 9), (tag, W, L)
                assert (cp(W, go, ge, tab.ctypes.data, L) > 0) == sg.cp_value_range_ok(W, L, go, ge, m), (tag, W, L)
            plan = sg.pk_plan(W, go, ge, m)
            spread, rebase = ctypes.c_int(-1), ctypes.c_int(-1)
            got = pk(W, go, ge, tab.ctypes.data, ctypes.byref(spread), ctypes.byref(rebase))
            assert bool(got) == plan.admitted, (tag, W, plan)
            if plan.admitted:
                assert (spread.value, rebase.value) == (plan.spread, sg.PK_REBASE), (tag, W, spread.value, plan)
        # the entry decides the packed rows' admission at W = 80 (total 32,000 is the limit), not at W = 14
        assert sg.pk_plan(14, go, ge, m).admitted
        without = sg.pk_plan(80, *ct.matrix_of("distinct")[1:], base)
        assert without.admitted and sg.pk_plan(80, go, ge, m).total > without.total + 10000, tag
