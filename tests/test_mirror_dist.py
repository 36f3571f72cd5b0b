"""The Python mirror of the distance sink without a device, with the stand-in library of tests/test_mirror_records.py: the sink
sets and resets ramx_set_dist_sink, a hand-made ramx_dist record is copied out, the keyword forms of extend_alignment /
extend_batch are followed down to the setter, the result comes last in the tuple, and a call without `dist` makes exactly the
calls it made before the keyword existed."""
import ctypes as C

import numpy as np
import pytest

from repeatafterme_amd import _lib, extend
from repeatafterme_amd.datamodel import ALN_END_DTYPE, COPY_DIST_DTYPE, PERIOD_DTYPE

import test_mirror_records as mr
from test_mirror_records import addr, deliver, numbered, one_family, params, same, scribble

SETTER = dict(mr.SETTER, dist="ramx_set_dist_sink")
REC = dict(mr.REC, dist=_lib.DistRec)
CB = dict(mr.CB, dist=_lib.DIST_CB)
DEFAULT, GIVEN = (1, 256), (20, 64)


class FakeLib(mr.FakeLib):
    """mr.FakeLib that also knows the distance sink"""

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
                self.fire(reversed(range(args[2])))
            return 0
        return call

    def fire(self, families):
        self.active = list(self.sinks)
        for f in families:
            for kind, cb in self.sinks.items():
                rec = REC[kind]()
                rec.family = f
                cb(C.byref(rec), None)


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    return lib


def check_entry_and_exit(fake, sink, given):
    entry, exit_ = fake.of("ramx_set_dist_sink")
    assert entry[0] is sink._cb and isinstance(entry[0], _lib.DIST_CB) and entry[1] is None
    assert entry[2:] == given and [type(x) for x in entry[2:]] == [int, int]
    assert isinstance(exit_[0], _lib.DIST_CB) and not exit_[0] and exit_[1] is None
    assert exit_[2:] == DEFAULT and [type(x) for x in exit_[2:]] == [int, int]


def test_sink_sets_and_resets(fake):
    sink = extend._DistSink(GIVEN)
    with sink as inside:
        assert inside is sink and len(fake.of("ramx_set_dist_sink")) == 1
    assert len(fake.calls) == 2
    check_entry_and_exit(fake, sink, GIVEN)


def test_sink_resets_on_exception(fake):
    sink = extend._DistSink(GIVEN)
    with pytest.raises(KeyError):
        with sink:
            raise KeyError("inside the block")
    assert len(fake.calls) == 2
    check_entry_and_exit(fake, sink, GIVEN)


def test_dist_record_is_copied_out():
    n, c = 4, 3
    cons, core, ends = np.array([2, 0, 3], np.int8), np.array([7, 5, 6, 4], np.int32), numbered(n, ALN_END_DTYPE, 3)
    copies, dist = np.array([0, 2, 3], np.int32), numbered(c * c, COPY_DIST_DTYPE, 11)
    want = (cons.copy(), core.copy(), ends.copy(), copies.copy(), dist.copy().reshape(c, c))
    ds = deliver(extend._DistSink(), _lib.DistRec(1, 5, 3, n, c, addr(cons), addr(core), addr(ends), addr(copies), addr(dist)))
    for again in (False, True):
        assert (ds.direction, ds.family) == (1, 5)
        assert same(ds.cons, want[0]) and same(ds.core_index, want[1]) and same(ds.ends, want[2]) and same(ds.copies, want[3])
        assert ds.dist.shape == (c, c) and same(ds.dist, want[4])
        scribble(cons, core, ends, copies, dist)            # every kept array is a copy


def test_dist_record_empty():
    ds = deliver(extend._DistSink(), _lib.DistRec(0, 2, 0, 0, 0, None, None, None, None, None))
    assert ds.family == 2 and same(ds.copies, np.zeros(0, np.int32)) and same(ds.dist, np.zeros((0, 0), COPY_DIST_DTYPE))
    assert same(ds.ends, np.zeros(0, ALN_END_DTYPE)) and same(ds.cons, np.zeros(0, np.int8))


def test_keyword_forms(fake):
    cores, seq, master = one_family()
    extend.extend_alignment(1, cores, seq, master, params(), dist=True)
    extend.extend_alignment(1, cores, seq, master, params(), dist=(1, 256))
    extend.extend_alignment(1, cores, seq, master, params(), dist=(30, 2048))
    a, _, b, _, c, _ = fake.of("ramx_set_dist_sink")
    assert a[2:] == b[2:] == (1, 256) and c[2:] == (30, 2048)
    fams = [one_family(n) for n in (1, 2)]
    extend.extend_batch(0, fams, params(), dist=(5, 7))
    assert fake.of("ramx_set_dist_sink")[6][2:] == (5, 7) and fake.of("ramx_set_dist_sink")[7][2:] == DEFAULT


def test_the_result_is_last_with_and_without_period(fake):
    cores, seq, master = one_family()
    res = extend.extend_alignment(1, cores, seq, master, params(), dist=True)
    assert [type(r).__name__ for r in res] == ["RunInfo", "Dist"]
    res = extend.extend_alignment(0, cores, seq, master, params(), profile=True, align=True, refine=5, copies=True, linkage=True,
                                  subfam=True, cpg=6, period=True, dist=GIVEN)
    assert fake.set_order[-8:] == ["dist"] + mr.ENTER_ORDER and fake.active == ["dist"] + mr.ENTER_ORDER and not fake.sinks
    assert [type(r).__name__ for r in res[1:8]] == mr.RESULT_TYPES
    assert len(res) == 10 and res[8].dtype == PERIOD_DTYPE and type(res[9]).__name__ == "Dist"
    names = [n for n, _ in fake.calls]
    assert names.index("ramx_period_flat") < len(names) - 1 and names[-1] == "ramx_set_dist_sink"     # the reset comes behind the periodicity
    res = extend.extend_alignment(1, cores, seq, master, params(), copies=True, dist=True)
    assert [type(r).__name__ for r in res] == ["RunInfo", "Copies", "Dist"]
    fams = [one_family(n) for n in (1, 2, 3)]
    res = extend.extend_batch(1, fams, params(), copies=True, period=True, dist=True)
    assert len(res) == 4 and [type(r).__name__ for r in res[1]] == ["Copies"] * 3 and all(r.dtype == PERIOD_DTYPE for r in res[2])
    assert [type(r).__name__ for r in res[3]] == ["Dist"] * 3 and [r.family for r in res[3]] == [0, 1, 2]
    res = extend.extend_batch(1, fams, params(), dist=True)
    assert len(res) == 2 and [r.family for r in res[1]] == [0, 1, 2]


def test_a_call_without_dist_makes_the_calls_it_made_before(fake):
    cores, seq, master = one_family()
    extend.extend_alignment(1, cores, seq, master, params())
    assert [n for n, _ in fake.calls] == ["ramx_extend_flat"]
    fake.calls.clear()
    extend.extend_alignment(0, cores, seq, master, params(), profile=True, align=True, refine=5, copies=True, linkage=True, subfam=True,
                            cpg=6, period=True)
    want = [mr.SETTER[k] for k in mr.ENTER_ORDER] + ["ramx_extend_flat"] + [mr.SETTER[k] for k in reversed(mr.ENTER_ORDER)] + ["ramx_period_flat"]
    assert [n for n, _ in fake.calls] == want
    fake.calls.clear()
    extend.extend_batch(1, [one_family(1)], params(), dist=None)
    assert [n for n, _ in fake.calls] == ["ramx_extend_batch"]


def test_extend_batch_refuses_a_missing_record(fake, monkeypatch):
    fams = [one_family(1), one_family(1)]
    monkeypatch.setattr(fake, "fire", lambda families: FakeLib.fire(fake, [0, 0]))
    with pytest.raises(AssertionError):
        extend.extend_batch(1, fams, params(), dist=True)
    assert not fake.sinks
