"""Cross-family overlap of the extended consensi (C-ABI include/ramx_xfam.h): the gapped local alignment of pairs of sequences on
the device, the candidate pairs by shared K-mers, the groups of linked families, and the three chained.  Sequences are arrays of
library codes (0..7 are bases, class code & 3; anything else is class 4); records are TERM_DTYPE."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .datamodel import SEQ_PAIR_DTYPE, TERM_DTYPE, PairParams, XfamLinkParams


def _flatten(seqs: Sequence[np.ndarray]):
    """-> (codes int8, seq_off int64 [n + 1])"""
    arrs = [np.ascontiguousarray(s, dtype=np.int8).reshape(-1) for s in seqs]
    off = np.zeros(len(arrs) + 1, np.int64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs])
    codes = np.concatenate(arrs) if arrs else np.zeros(0, np.int8)
    return np.ascontiguousarray(codes, dtype=np.int8), off


def _pairs_array(pairs) -> np.ndarray:
    if isinstance(pairs, np.ndarray) and pairs.dtype == SEQ_PAIR_DTYPE:
        return np.ascontiguousarray(pairs)
    out = np.zeros(len(pairs), SEQ_PAIR_DTYPE)
    for i, p in enumerate(pairs):
        out[i]["a"], out[i]["b"], out[i]["inverted"] = int(p[0]), int(p[1]), int(p[2])
        out[i]["reserved"] = int(p[3]) if len(p) > 3 else 0
    return out


def _cparams(params: Optional[PairParams]) -> _lib.PairParams:
    p = PairParams() if params is None else params
    return _lib.PairParams(int(p.match), int(p.mismatch), int(p.gap), int(p.min_score))


def _ptr(a: np.ndarray):
    return a.ctypes.data if a.size else None


def seq_pair_host(a, b, inverted: int = 0, params: Optional[PairParams] = None) -> np.ndarray:
    """The record of one pair on the host (ramx_seq_pair_host) -> TERM_DTYPE [1]."""
    a = np.ascontiguousarray(a, dtype=np.int8)
    b = np.ascontiguousarray(b, dtype=np.int8)
    out = np.zeros(1, TERM_DTYPE)
    cp = _cparams(params)
    _lib.check(_lib.lib().ramx_seq_pair_host(_ptr(a), len(a), _ptr(b), len(b), int(inverted), C.byref(cp), out.ctypes.data),
               "ramx_seq_pair_host")
    return out


def seq_pairs(seqs, pairs, params: Optional[PairParams] = None, device=None, timing: bool = False):
    """One record per pair, in pair order, on the device (ramx_dev_seq_pairs).  pairs: SEQ_PAIR_DTYPE, or tuples (a, b,
    inverted); device: a Device, or None for the process-wide session.  -> TERM_DTYPE [n_pairs] (with timing: and the
    alignment kernels' milliseconds)."""
    codes, off = _flatten(seqs)
    pa = _pairs_array(pairs)
    out = np.zeros(len(pa), TERM_DTYPE)
    cp = _cparams(params)
    ms = C.c_double(0.0)
    handle = device._h if device is not None else None
    _lib.check(_lib.lib().ramx_dev_seq_pairs(handle, _ptr(codes), off.ctypes.data, len(off) - 1, _ptr(pa), len(pa), C.byref(cp),
                                             _ptr(out), C.byref(ms) if timing else None), "ramx_dev_seq_pairs")
    return (out, ms.value) if timing else out


def candidates(seqs, owner, K: int = 16, within: bool = False, cap: Optional[int] = None) -> np.ndarray:
    """The pairs worth aligning (ramx_xfam_candidates) -> SEQ_PAIR_DTYPE; with cap, the first cap of them."""
    codes, off = _flatten(seqs)
    own = np.ascontiguousarray(owner, dtype=np.int32)
    if len(own) != len(off) - 1:
        raise ValueError("one owner per sequence")
    L = _lib.lib()
    n = _lib.check(L.ramx_xfam_candidates(_ptr(codes), off.ctypes.data, len(own), _ptr(own), int(K), int(bool(within)), None, 0),
                   "ramx_xfam_candidates")
    room = n if cap is None else min(n, int(cap))
    out = np.zeros(room, SEQ_PAIR_DTYPE)
    if room:
        _lib.check(L.ramx_xfam_candidates(_ptr(codes), off.ctypes.data, len(own), _ptr(own), int(K), int(bool(within)),
                                          out.ctypes.data, room), "ramx_xfam_candidates")
    return out


def groups(pairs, records, owner, n_families: int, link: Optional[XfamLinkParams] = None):
    """Which records count and which families they join (ramx_xfam_groups) -> (counts int32 [n_pairs], group int32
    [n_families])."""
    pa = _pairs_array(pairs)
    rec = np.ascontiguousarray(records, dtype=TERM_DTYPE)
    if len(rec) != len(pa):
        raise ValueError("one record per pair")
    own = np.ascontiguousarray(owner, dtype=np.int32)
    lk = XfamLinkParams() if link is None else link
    cl = _lib.XfamLinkParams(int(lk.min_columns), int(lk.min_permille))
    counts = np.zeros(len(pa), np.int32)
    group = np.zeros(int(n_families), np.int32)
    _lib.check(_lib.lib().ramx_xfam_groups(_ptr(pa), _ptr(rec), len(pa), _ptr(own), int(n_families), C.byref(cl), _ptr(counts),
                                           _ptr(group)), "ramx_xfam_groups")
    return counts, group


def compare(seqs, owner, n_families: Optional[int] = None, K: int = 16, within: bool = False,
            params: Optional[PairParams] = None, link: Optional[XfamLinkParams] = None, device=None):
    """candidates -> seq_pairs -> groups.  -> (records, pairs, counts, group)."""
    own = np.ascontiguousarray(owner, dtype=np.int32)
    nf = int(own.max()) + 1 if n_families is None and len(own) else int(n_families or 0)
    pa = candidates(seqs, own, K=K, within=within)
    rec = seq_pairs(seqs, pa, params, device=device)
    counts, group = groups(pa, rec, own, nf, link)
    return rec, pa, counts, group


def write_tsv(path, names, sides, lengths, pairs, records, counts, owner, group, labels=None) -> str:
    """The cross-family file as RAMExtend -outxfam writes it: one header line, one line per record with a score in pair order,
    one #group line per component.  names[s], sides[s], lengths[s]: file, 'left' / 'right' / 'all' and length of sequence s;
    labels[f]: what stands for family f (its index if None).  b_from..b_to are in B's own reading coordinates whatever the
    orientation.  -> the summary line."""
    own = np.asarray(owner)
    lab = [str(f) for f in range(len(group))] if labels is None else [str(x) for x in labels]
    n_rec = n_link = 0
    with open(path, "w") as fh:
        fh.write("#family_a\tranges_a\tside_a\tfamily_b\tranges_b\tside_b\torient\tscore\ta_from\ta_to\tlen_a\tb_from\tb_to\tlen_b\t"
                 "matches\tcolumns\tidentity\tlink\n")
        for p, r, c in zip(pairs, records, counts):
            if r["score"] <= 0:
                continue
            a, b, inv = int(p["a"]), int(p["b"]), int(p["inverted"])
            nb = int(lengths[b])
            b_from, b_to = (int(r["b_start"]), int(r["b_end"])) if not inv else (nb - 1 - int(r["b_end"]), nb - 1 - int(r["b_start"]))
            link = int(bool(c) and own[a] != own[b])
            n_rec += 1
            n_link += link
            # three decimals, rounded half up in integers as the command line does
            ident = (2000 * int(r["matches"]) + int(r["columns"])) // (2 * int(r["columns"]))
            fh.write(f"{lab[own[a]]}\t{names[a]}\t{sides[a]}\t{lab[own[b]]}\t{names[b]}\t{sides[b]}\t{'-' if inv else '+'}\t{int(r['score'])}\t"
                     f"{int(r['a_start'])}\t{int(r['a_end'])}\t{int(lengths[a])}\t{b_from}\t{b_to}\t{nb}\t{int(r['matches'])}\t"
                     f"{int(r['columns'])}\t{ident // 1000}.{ident % 1000:03d}\t{link}\n")
        n_big = 0
        for g in sorted(set(int(x) for x in group)):
            members = [f for f in range(len(group)) if int(group[f]) == g]
            n_big += len(members) > 1
            fh.write(f"#group\t{lab[g]}\t{len(members)}\t{','.join(lab[f] for f in members)}\n")
    return f"xfam: {len(pairs)} candidates, {n_rec} records, {n_link} links, {n_big} groups with more than one family"
