"""The Python mirror of the seam-1 sinks without a device: hand-made ctypes records go straight to the callback object a sink
hands to the library (the C-side twin is tools/host_asan/cli_outputs_main.c), the setter calls of every sink are recorded on a
stand-in for the library object, and the keyword forms of extend_alignment / extend_batch are followed down to those calls."""
import ctypes as C

import numpy as np
import pytest

from repeatafterme_amd import _lib, extend
from repeatafterme_amd.datamodel import (ALN_END_DTYPE, ALN_NONE, COL_PROFILE_DTYPE, COPY_STATS_DTYPE, DINUC_DTYPE, FLANK_DTYPE, PERIOD_DTYPE,
                                         PILEUP_DTYPE, PLANE_DTYPE, CoreSet, ExtendParams, PeriodParams)

# ---- the private names this file reaches: a sink by its keyword, with the arguments its setter takes behind callback and user ----

_SINK_CLASSES = {"profile": "_ProfileSink", "align": "_AlignSink", "refine": "_RefineSink", "cpg": "_CpgSink", "copies": "_CopiesSink",
                 "linkage": "_LinkageSink", "subfam": "_SubfamSink"}


def make_sink(kind, *args):
    """-> the sink: a context manager with `got` (the records kept) and `_cb` (the callback object the library is handed)"""
    cls = getattr(extend, _SINK_CLASSES[kind])
    return cls(args) if kind in ("linkage", "subfam") else cls(*args)


SETTER = {"profile": "ramx_set_profile_sink", "align": "ramx_set_align_sink", "refine": "ramx_set_refine_sink", "cpg": "ramx_set_cpg_sink",
          "copies": "ramx_set_copies_sink", "linkage": "ramx_set_linkage_sink", "subfam": "ramx_set_subfam_sink"}
REC = {"profile": _lib.ProfileRec, "align": _lib.AlignRec, "refine": _lib.RefineRec, "cpg": _lib.CpgRec, "copies": _lib.CopiesRec,
       "linkage": _lib.LinkageRec, "subfam": _lib.SubfamRec}
CB = {"profile": _lib.PROFILE_CB, "align": _lib.ALIGN_CB, "refine": _lib.REFINE_CB, "cpg": _lib.CPG_CB, "copies": _lib.COPIES_CB,
      "linkage": _lib.LINKAGE_CB, "subfam": _lib.SUBFAM_CB}
# what every setter is reset to when its block ends
DEFAULTS = {"profile": (), "align": (), "refine": (1,), "cpg": (1, 0), "copies": (), "linkage": (4, 100, 1024),
            "subfam": (4, 100, 1024, 3.0, 4, 8, 4, 10)}
GIVEN = {"profile": (), "align": (), "refine": (7,), "cpg": (6, -3), "copies": (), "linkage": (2, 50, 16),
         "subfam": (2, 50, 16, 1.5, 3, 5, 2, 6)}


# ---- hand-made records ----

def numbered(count, dtype, start=1):
    """`count` records of `dtype` whose bytes are all different from zero and from each other's"""
    out = np.zeros(count, dtype)
    raw = out.view(np.uint8).reshape(-1)
    raw[:] = (np.arange(len(raw)) * 7 + start) % 251 + 1
    return out


def addr(a):
    return a.ctypes.data if a is not None and a.size else None


def deliver(sink, rec):
    sink._cb(C.byref(rec), None)
    return sink.got[-1]


def scribble(*arrays):
    for a in arrays:
        a.view(np.uint8).reshape(-1)[:] = 0xA5


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_align_record_stride_wider_than_flanks():
    rows, n, stride = 3, 2, 5
    cons = np.array([2, 0, 3], np.int8)
    flanks, core, ends = numbered(n, FLANK_DTYPE), np.array([4, 9], np.int32), numbered(n, ALN_END_DTYPE, 3)
    idx = (100 + np.arange(rows * stride)).astype(np.int32)
    ins = (500 + np.arange(rows * stride)).astype(np.int32)
    want = (cons.copy(), flanks.copy(), core.copy(), ends.copy())
    sink = make_sink("align")
    al = deliver(sink, _lib.AlignRec(1, 5, rows, n, stride, addr(cons), addr(flanks), addr(core), addr(ends), addr(idx), addr(ins)))
    for again in (False, True):
        assert (al.direction, al.family) == (1, 5)
        assert same(al.cons, want[0]) and same(al.flanks, want[1]) and same(al.core_index, want[2]) and same(al.ends, want[3])
        assert al.col_idx.shape == al.col_ins.shape == (rows, n) and al.col_idx.dtype == al.col_ins.dtype == np.int32
        for r in range(rows):
            for i in range(n):
                assert al.col_idx[r, i] == 100 + r * stride + i and al.col_ins[r, i] == 500 + r * stride + i
        scribble(cons, flanks, core, ends, idx, ins)       # every kept array is a copy
    assert len(sink.got) == 1


def test_align_record_without_columns():
    rows, n = 3, 2
    cons, flanks, core, ends = np.array([2, 0, 3], np.int8), numbered(n, FLANK_DTYPE), np.array([4, 9], np.int32), numbered(n, ALN_END_DTYPE)
    al = deliver(make_sink("align"), _lib.AlignRec(0, 0, rows, n, 5, addr(cons), addr(flanks), addr(core), addr(ends), None, None))
    assert al.col_idx.shape == al.col_ins.shape == (rows, n)
    assert (al.col_idx == ALN_NONE).all() and (al.col_ins == 0).all()
    assert same(al.cons, cons) and same(al.ends, ends)


def test_align_record_empty():
    al = deliver(make_sink("align"), _lib.AlignRec(0, 2, 0, 0, 0, None, None, None, None, None, None))
    assert al.family == 2
    assert same(al.cons, np.zeros(0, np.int8)) and same(al.flanks, np.zeros(0, FLANK_DTYPE)) and same(al.core_index, np.zeros(0, np.int32))
    assert same(al.ends, np.zeros(0, ALN_END_DTYPE))
    assert same(al.col_idx, np.zeros((0, 0), np.int32)) and same(al.col_ins, np.zeros((0, 0), np.int32))


def test_profile_record_without_columns():
    core, last = np.array([3, 1, 2], np.int32), np.array([-1, 8, 0], np.int32)
    want = (core.copy(), last.copy())
    pr = deliver(make_sink("profile"), _lib.ProfileRec(1, 4, 0, 0, 3, None, addr(core), addr(last)))
    for again in (False, True):
        assert (pr.direction, pr.family, pr.ret) == (1, 4, 0)
        assert same(pr.cols, np.zeros(0, COL_PROFILE_DTYPE)) and same(pr.core_index, want[0]) and same(pr.last_uncapped_row, want[1])
        scribble(core, last)


def test_profile_record_with_columns():
    cols, core, last = numbered(4, COL_PROFILE_DTYPE), np.array([0], np.int32), np.array([3], np.int32)
    want = cols.copy()
    pr = deliver(make_sink("profile"), _lib.ProfileRec(0, 0, 4, 2, 1, addr(cols), addr(core), addr(last)))
    scribble(cols)
    assert pr.ret == 2 and same(pr.cols, want) and pr.core_index.tolist() == [0] and pr.last_uncapped_row.tolist() == [3]


def test_linkage_record_without_planes():
    cons, cols = np.array([1, 1], np.int8), numbered(2, PILEUP_DTYPE)
    lk = deliver(make_sink("linkage", *DEFAULTS["linkage"]), _lib.LinkageRec(1, 0, 2, 0, addr(cons), addr(cols), None, None))
    assert lk.co.shape == (0, 0) and lk.co.dtype == np.int32 and same(lk.planes, np.zeros(0, PLANE_DTYPE))
    assert same(lk.cons, cons) and same(lk.cols, cols)


def test_linkage_record_with_planes():
    cons, cols = np.array([1, 1], np.int8), numbered(2, PILEUP_DTYPE)
    planes, co = numbered(2, PLANE_DTYPE), np.array([11, 12, 21, 22], np.int32)
    want = (cols.copy(), planes.copy())
    lk = deliver(make_sink("linkage", *DEFAULTS["linkage"]), _lib.LinkageRec(0, 3, 2, 2, addr(cons), addr(cols), addr(planes), addr(co)))
    for again in (False, True):
        assert (lk.direction, lk.family) == (0, 3) and lk.cons.tolist() == [1, 1]
        assert same(lk.cols, want[0]) and same(lk.planes, want[1])
        assert lk.co.dtype == np.int32 and lk.co.tolist() == [[11, 12], [21, 22]]
        scribble(cons, cols, planes, co)


def test_subfam_record_shapes_and_groups():
    V, K, P, n, rows = 2, 3, 3, 2, 4
    cons, flanks, core = np.array([0, 1, 2, 3], np.int8), numbered(n, FLANK_DTYPE), np.array([5, 6], np.int32)
    planes, labels = numbered(P, PLANE_DTYPE), np.array([2, 0], np.int32)
    pats = (1 + np.arange(V * K)).astype(np.uint8)
    cnt = (10 + np.arange(K * P)).astype(np.int32)
    size = np.array([1, 0, 1], np.int32)
    dist = (40 + np.arange(n * K)).astype(np.int32)
    rcons, rcols = np.array([3, 3, 1], np.int8), numbered(3, PILEUP_DTYPE, 9)
    groups = (_lib.SubfamGroup * 2)(_lib.SubfamGroup(0, 7, 3, 2, 1, addr(rcons), addr(rcols)), _lib.SubfamGroup(2, 5, 0, 0, 0, None, None))
    want = (flanks.copy(), planes.copy(), rcols.copy())
    sf = deliver(make_sink("subfam", *DEFAULTS["subfam"]),
                 _lib.SubfamRec(1, 1, rows, n, P, V, K, 6, 1, 2, addr(cons), addr(flanks), addr(core), addr(planes), addr(labels), addr(pats),
                                addr(cnt), addr(size), addr(dist), groups))
    for again in (False, True):
        assert (sf.direction, sf.family, sf.iterations, sf.converged) == (1, 1, 6, 1)
        assert sf.cons.tolist() == [0, 1, 2, 3] and same(sf.flanks, want[0]) and sf.core_index.tolist() == [5, 6]
        assert same(sf.planes, want[1]) and sf.labels.tolist() == [2, 0] and sf.size.tolist() == [1, 0, 1]
        assert sf.patterns.dtype == np.uint8 and sf.patterns.tolist() == [[1, 2, 3], [4, 5, 6]]                     # [V][K]
        assert sf.cnt.dtype == np.int32 and sf.cnt.tolist() == [[10, 11, 12], [13, 14, 15], [16, 17, 18]]           # [K][P]
        assert sf.dist.dtype == np.int32 and sf.dist.tolist() == [[40, 41, 42], [43, 44, 45]]                       # [n][K]
        g0, g2 = sf.groups
        assert (g0.group, g0.size, g0.replays, g0.converged) == (0, 7, 2, 1)
        assert g0.refined_cons.tolist() == [3, 3, 1] and same(g0.refined_cols, want[2])
        assert (g2.group, g2.size, g2.replays, g2.converged) == (2, 5, 0, 0)
        assert same(g2.refined_cons, np.zeros(0, np.int8)) and same(g2.refined_cols, np.zeros(0, PILEUP_DTYPE))
        scribble(cons, flanks, core, planes, labels, pats, cnt, size, dist, rcons, rcols)
        groups[0].size = groups[0].group = -1


def test_refine_record():
    cons, cols = np.array([0, 3], np.int8), numbered(2, PILEUP_DTYPE)
    rcons, rcols = np.array([0, 2], np.int8), numbered(2, PILEUP_DTYPE, 5)
    want = (cols.copy(), rcols.copy())
    rf = deliver(make_sink("refine", 4), _lib.RefineRec(1, 2, 2, 2, 3, 1, 9, 0, addr(cons), addr(cols), addr(rcons), addr(rcols)))
    for again in (False, True):
        assert (rf.direction, rf.family, rf.replays, rf.converged) == (1, 2, 3, 1)
        assert rf.cons.tolist() == [0, 3] and rf.cons.dtype == np.int8 and same(rf.cols, want[0])
        assert rf.refined_cons.tolist() == [0, 2] and same(rf.refined_cols, want[1])
        scribble(cons, cols, rcons, rcols)


def test_cpg_record():
    cons, rcons = np.array([1, 2], np.int8), np.array([1, 0], np.int8)
    rcols, rdi = numbered(2, PILEUP_DTYPE), numbered(2, DINUC_DTYPE, 5)
    want = (rcols.copy(), rdi.copy())
    cr = deliver(make_sink("cpg", 4, 0), _lib.CpgRec(0, 1, 2, 2, 2, 0, 9, 1, addr(cons), addr(rcons), addr(rcols), addr(rdi)))
    for again in (False, True):
        assert (cr.direction, cr.family, cr.replays, cr.converged, cr.n_cpg) == (0, 1, 2, 0, 1)
        assert cr.cons.tolist() == [1, 2] and cr.refined_cons.tolist() == [1, 0]
        assert same(cr.refined_cols, want[0]) and same(cr.refined_di, want[1])
        scribble(cons, rcons, rcols, rdi)


def test_copies_record():
    cons, flanks, core = np.array([2, 2], np.int8), numbered(3, FLANK_DTYPE), np.array([0, 2, 1], np.int32)
    ends, stats = numbered(3, ALN_END_DTYPE), numbered(3, COPY_STATS_DTYPE, 5)
    want = (flanks.copy(), ends.copy(), stats.copy())
    cp = deliver(make_sink("copies"), _lib.CopiesRec(1, 0, 2, 3, addr(cons), addr(flanks), addr(core), addr(ends), addr(stats)))
    for again in (False, True):
        assert (cp.direction, cp.family) == (1, 0) and cp.cons.tolist() == [2, 2] and cp.core_index.tolist() == [0, 2, 1]
        assert same(cp.flanks, want[0]) and same(cp.ends, want[1]) and same(cp.stats, want[2])
        scribble(cons, flanks, core, ends, stats)


# ---- a stand-in for the library object: it records every call, and its extension entries answer every sink that is set ----

class FakeLib:
    def __init__(self):
        self.calls = []                  # (name, args)
        self.sinks = {}                  # kind -> callback, for the sinks that are set
        self.set_order = []              # kinds in the order their sinks were set
        self.active = []                 # kinds whose sinks were set at the last extension call

    def __getattr__(self, name):
        if not name.startswith("ramx_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            for kind, setter in SETTER.items():
                if name == setter:
                    assert isinstance(args[0], CB[kind]) and args[1] is None
                    if args[0]:
                        self.sinks[kind] = args[0]
                        self.set_order.append(kind)
                    else:
                        del self.sinks[kind]
            if name == "ramx_extend_flat":
                self.fire([0])
            if name == "ramx_extend_batch":
                self.fire(reversed(range(args[2])))         # the order of the records is not that of the families
            return 0
        return call

    def fire(self, families):
        self.active = list(self.sinks)
        for f in families:
            for kind, cb in self.sinks.items():
                rec = REC[kind]()
                rec.family = f
                cb(C.byref(rec), None)

    def of(self, name):
        return [a for n, a in self.calls if n == name]


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    return lib


def check_entry_and_exit(fake, kind, sink):
    entry, exit_ = fake.of(SETTER[kind])
    assert entry[0] is sink._cb and isinstance(entry[0], CB[kind]) and entry[1] is None
    assert entry[2:] == GIVEN[kind] and [type(x) for x in entry[2:]] == [type(x) for x in DEFAULTS[kind]]
    assert isinstance(exit_[0], CB[kind]) and not exit_[0] and exit_[1] is None
    assert exit_[2:] == DEFAULTS[kind] and [type(x) for x in exit_[2:]] == [type(x) for x in DEFAULTS[kind]]


@pytest.mark.parametrize("kind", list(SETTER))
def test_sink_sets_and_resets(fake, kind):
    sink = make_sink(kind, *GIVEN[kind])
    with sink as inside:
        assert inside is sink and len(fake.of(SETTER[kind])) == 1
    assert len(fake.calls) == 2
    check_entry_and_exit(fake, kind, sink)


@pytest.mark.parametrize("kind", list(SETTER))
def test_sink_resets_on_exception(fake, kind):
    sink = make_sink(kind, *GIVEN[kind])
    with pytest.raises(KeyError):
        with sink:
            raise KeyError("inside the block")
    assert len(fake.calls) == 2
    check_entry_and_exit(fake, kind, sink)


def test_refine_sink_stays_importable(fake):
    """tests/test_gpu_sink_paths.py sets this one by hand around extend_batch"""
    with extend._RefineSink(7) as rs:
        fake.fire([0])
    assert len(rs.got) == 1 and rs.got[0].family == 0
    assert fake.of("ramx_set_refine_sink")[0][2:] == (7,) and fake.of("ramx_set_refine_sink")[1][2:] == (1,)


# ---- the keyword forms, followed down to the setter calls ----

L_ = 8


def one_family(n=2):
    cores = CoreSet(*(np.zeros(n, np.int64) for _ in range(4)), *(np.zeros(n, np.int8) for _ in range(3)))
    return cores, np.zeros(40, np.int8), np.zeros(2 * L_ + 2, np.int8)


def params():
    return ExtendParams(L=L_, matrix=np.zeros(100 * 100, np.int32))


def set_args(fake, kind):
    """the arguments the sink of `kind` was set with, behind callback and user"""
    return fake.of(SETTER[kind])[0][2:]


ENTER_ORDER = ["cpg", "subfam", "linkage", "copies", "refine", "align", "profile"]
RESULT_TYPES = ["Profile", "Alignment", "Refinement", "Copies", "Linkage", "Subfamilies", "CpgRefinement"]


def test_extend_alignment_plain(fake):
    cores, seq, master = one_family()
    info = extend.extend_alignment(1, cores, seq, master, params())
    assert isinstance(info, extend.RunInfo)
    assert [n for n, _ in fake.calls] == ["ramx_extend_flat"]
    a = fake.of("ramx_extend_flat")[0]
    assert a[0] == 1 and a[2] == seq.ctypes.data and a[3] == len(seq) and a[4] == master.ctypes.data
    fc = a[1]._obj
    assert fc.n == cores.n
    for k in ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext", "right_ext", "left_len", "right_len", "score"):
        assert getattr(fc, k) == getattr(cores, k).ctypes.data, k


def test_extend_alignment_all_sinks(fake):
    cores, seq, master = one_family()
    res = extend.extend_alignment(0, cores, seq, master, params(), profile=True, align=True, refine=5, copies=True, linkage=True,
                                  subfam=True, cpg=6, period=True)
    assert fake.set_order == ENTER_ORDER and fake.active == ENTER_ORDER     # cpg outermost, profile innermost, all set at the call
    assert not fake.sinks                                                   # ... and none afterwards
    assert isinstance(res, tuple) and isinstance(res[0], extend.RunInfo)
    assert [type(r).__name__ for r in res[1:8]] == RESULT_TYPES
    assert len(res) == 9 and res[8].dtype == PERIOD_DTYPE and res[8].shape == (cores.n,)
    assert set_args(fake, "refine") == (5,) and set_args(fake, "cpg") == (6, 0)
    assert set_args(fake, "linkage") == DEFAULTS["linkage"] and set_args(fake, "subfam") == DEFAULTS["subfam"]
    for kind in ENTER_ORDER:
        exit_ = fake.of(SETTER[kind])[1]
        assert not exit_[0] and exit_[2:] == DEFAULTS[kind]
    names = [n for n, _ in fake.calls]
    assert names.index("ramx_period_flat") == len(names) - 1               # after every sink is reset
    pf = fake.of("ramx_period_flat")[0]
    assert pf[3] == 0                                                      # which = direction


def test_extend_alignment_some_sinks(fake):
    cores, seq, master = one_family()
    res = extend.extend_alignment(1, cores, seq, master, params(), align=True, linkage=(2, 50, 16))
    assert [type(r).__name__ for r in res] == ["RunInfo", "Alignment", "Linkage"]
    assert fake.set_order == ["linkage", "align"] and set_args(fake, "linkage") == (2, 50, 16)
    res = extend.extend_alignment(1, cores, seq, master, params(), profile=True)
    assert [type(r).__name__ for r in res] == ["RunInfo", "Profile"]


def test_keyword_forms(fake):
    cores, seq, master = one_family()
    extend.extend_alignment(1, cores, seq, master, params(), linkage=True)
    extend.extend_alignment(1, cores, seq, master, params(), linkage=(4, 100, 1024))
    a, _, b, _ = fake.of(SETTER["linkage"])
    assert a[2:] == b[2:] == (4, 100, 1024)
    extend.extend_alignment(1, cores, seq, master, params(), subfam=True)
    extend.extend_alignment(1, cores, seq, master, params(), subfam=(4, 100, 1024, 3, 4, 8, 4, 10))
    a, _, b, _ = fake.of(SETTER["subfam"])
    assert a[2:] == b[2:] == DEFAULTS["subfam"] and [type(x) for x in b[2:]] == [int, int, int, float, int, int, int, int]
    extend.extend_alignment(1, cores, seq, master, params(), cpg=3)
    extend.extend_alignment(1, cores, seq, master, params(), cpg=(3, 0))
    extend.extend_alignment(1, cores, seq, master, params(), cpg=(3, -2))
    a, _, b, _, c, _ = fake.of(SETTER["cpg"])
    assert a[2:] == b[2:] == (3, 0) and c[2:] == (3, -2)
    r1 = extend.extend_alignment(1, cores, seq, master, params(), period=True)
    r2 = extend.extend_alignment(1, cores, seq, master, params(), period=PeriodParams())
    extend.extend_alignment(1, cores, seq, master, params(), period=PeriodParams(pmax=7, mm=2, min_score=5))
    assert len(r1) == len(r2) == 2
    a, b, c = (x[4]._obj for x in fake.of("ramx_period_flat"))
    assert (a.pmax, a.mm, a.min_score, a.reserved) == (b.pmax, b.mm, b.min_score, b.reserved) == (1024, 3, 16, 0)
    assert (c.pmax, c.mm, c.min_score, c.reserved) == (7, 2, 5, 0)
    assert all(x[3] == 1 for x in fake.of("ramx_period_flat"))


def test_extend_batch_orders_by_family(fake):
    fams = [one_family(n) for n in (1, 2, 3)]
    res = extend.extend_batch(1, fams, params(), profile=True, align=True, copies=True, linkage=True, subfam=True, period=True)
    assert fake.set_order == ["subfam", "linkage", "copies", "align", "profile"] and not fake.sinks
    assert isinstance(res, tuple) and len(res) == 7
    assert len(res[0]) == 3 and all(isinstance(i, extend.RunInfo) for i in res[0])
    for recs, name in zip(res[1:6], ["Profile", "Alignment", "Copies", "Linkage", "Subfamilies"]):
        assert [type(r).__name__ for r in recs] == [name] * 3 and [r.family for r in recs] == [0, 1, 2]
    assert [len(r) for r in res[6]] == [1, 2, 3] and all(r.dtype == PERIOD_DTYPE for r in res[6])
    arr, n = fake.of("ramx_extend_batch")[0][1:3]
    assert n == 3
    for i, (cores, seq, master) in enumerate(fams):
        assert (arr[i].cores.n, arr[i].sequence, arr[i].seq_len, arr[i].master) == (cores.n, seq.ctypes.data, len(seq), master.ctypes.data)
        assert arr[i].cores.left_pos == cores.left_pos.ctypes.data and arr[i].cores.score == cores.score.ctypes.data
    assert fake.of("ramx_period_batch")[0][2] == 1
    infos = extend.extend_batch(0, fams, params())
    assert isinstance(infos, list) and len(infos) == 3


def test_extend_batch_refuses_a_missing_record(fake, monkeypatch):
    fams = [one_family(1), one_family(1)]
    monkeypatch.setattr(fake, "fire", lambda families: FakeLib.fire(fake, [0, 0]))       # two records of family 0, none of family 1
    with pytest.raises(AssertionError):
        extend.extend_batch(1, fams, params(), copies=True)
    assert not fake.sinks                                                                  # the sink is reset all the same


def test_extend_alignment_refuses_a_second_record(fake, monkeypatch):
    cores, seq, master = one_family()
    monkeypatch.setattr(fake, "fire", lambda families: FakeLib.fire(fake, [0, 0]))
    with pytest.raises(AssertionError):
        extend.extend_alignment(1, cores, seq, master, params(), align=True)
    assert not fake.sinks
