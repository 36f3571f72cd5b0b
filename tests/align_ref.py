"""Reference side of the per-copy alignments (a helper, not a test): a CPU walker over the oracle's single-row function, a
rescorer of the walked path, and a renderer of the `-outaln` text.

The walker restates the contract of include/ramx.h (ramx_aln_end, ramx_dev_align) on the oracle's cells: the band of one flank
is stepped along a given consensus with po.oracle_nw_row, every row's (substitution, gap) cells are kept, and the path is
walked back from the end cell with the reference's own comparisons (bnw_extend.c:896-904, 950-956, 976-984, 1007, 1015)."""
import numpy as np

from oracle import pyoracle as po

DELETED = -2 ** 31
NONE = -2 ** 31 + 1
_COMPL = {0: 3, 1: 2, 2: 1, 3: 0, 4: 7, 5: 6, 6: 5, 7: 4}


class Flank:
    """One extendable core seen from one direction: where flank position t lies in the library, and which cells are inside."""

    def __init__(self, direction, cores, n, W):
        self.lp, self.rp, self.orient = int(cores.left_pos[n]), int(cores.right_pos[n]), int(cores.orient[n])
        self.lo, self.up = int(cores.lower[n]), int(cores.upper[n])
        self.W = W
        if direction:
            self.start = self.rp - 1 if self.orient else self.rp + 1
        else:
            self.start = self.lp + 1 if self.orient else self.lp - 1
        self.sgn = -1 if direction == self.orient else 1

    def inside(self, t):
        so = self.sgn * t
        if self.start < self.W and so < 0 and -so > self.start:      # before the library's first base (bnw_extend.c:843-868)
            return False
        return self.lo <= self.start + so <= self.up

    def base(self, t, sequence):
        """The base code at flank position t as the alignment sees it (complemented on the reverse strand); 99 outside."""
        si = self.start + self.sgn * t
        if si < 0 or si >= len(sequence):
            return 99
        b = int(sequence[si])
        return _COMPL.get(b, 99) if self.orient else b


def forward(direction, cores, n, sequence, p, cons):
    """Rows -1 .. len(cons)-1 of core n's band along cons: {row: [2W+1][2] (substitution, gap)}, the rows' best scores and
    indices (row + offset)."""
    W, B, go, ge = p.bandwidth, 2 * p.bandwidth + 1, p.gapopen, p.gapextn
    mat = np.ascontiguousarray(p.matrix, np.int32)
    seq = np.ascontiguousarray(sequence, np.int8)
    sc = np.zeros((2, 1, B, 2), np.int32)
    for j in range(B):
        sc[1, 0, j, :] = 0 if j == W else go + abs(j - W) * ge
    S = {-1: sc[1, 0].astype(np.int64)}
    best, idx = [], []
    for r in range(len(cons)):
        b, i = po.oracle_nw_row(direction, r, 0, 1, int(cons[r]), int(cores.left_pos[n]), int(cores.right_pos[n]), int(cores.orient[n]),
                                sc, int(cores.lower[n]), int(cores.upper[n]), seq, mat, go, ge, W)
        best.append(b)
        idx.append(i)
        S[r] = sc[r % 2, 0].astype(np.int64)
    return S, best, idx


def walk(direction, cores, n, sequence, p, cons):
    """-> dict: end_row, end_idx, score, start_idx, tail_ins, col_idx[rows], col_ins[rows], ops (path order: ('M', row, t),
    ('I', t), ('D', row)), origin (the path begins at the origin cell) and the counters the corpus checks look at."""
    W, go, ge, rows = p.bandwidth, p.gapopen, p.gapextn, len(cons)
    fl = Flank(direction, cores, n, W)
    S, best, idx = forward(direction, cores, n, sequence, p, cons)
    out = dict(end_row=-1, end_idx=-1, score=0, start_idx=0, tail_ins=0, col_idx=np.full(rows, NONE, np.int64),
               col_ins=np.zeros(rows, np.int64), ops=[], origin=False, row_best=best, row_best_idx=idx,
               n_ins=0, n_del=0, ties_state=0, ties_insdel=0, ties_open=0, early_end=0, gap_end=0, edge_end=0, bound_end=0)
    high, end_row = 0, -1
    for r in range(rows):                              # the first row above every earlier one, and above 0
        if best[r] > high:
            high, end_row = best[r], r
    if end_row < 0:
        return out
    out.update(end_row=end_row, end_idx=idx[end_row], score=high, early_end=int(end_row < rows - 1))
    r, j = end_row, idx[end_row] - end_row + W
    assert max(S[r][j]) == high
    gap = S[r][j][1] > S[r][j][0]
    out["gap_end"] = int(gap)
    ops, NEGI = [], -10 ** 15
    start = idx[end_row] + 1
    while True:
        t = j - W + r
        if r == -1:
            o = j - W
            for k in range(max(o, 0) - 1, -1, -1):
                ops.append(("I", k))
            start = min(o, 0)
            out["origin"] = (o == 0)
            out["bound_end"] = 1
            break
        if not fl.inside(t):
            assert S[r][j][0] == go + (r + 1) * ge, "a path may only leave the flank through a matrix-edge fill cell"
            for k in range(r, -1, -1):
                ops.append(("D", k))
            start = t + 1
            out["edge_end"] = 1
            break
        up = S[r - 1]
        if not gap:
            ops.append(("M", r, t))
            start = t
            if r - 1 >= 0 and fl.inside(t - 1) and up[j][1] == up[j][0]:
                out["ties_state"] += 1
            gap = up[j][1] > up[j][0]
            r -= 1
            continue
        d_open = d_ext = i_open = i_ext = NEGI
        if j < 2 * W:
            d_open, d_ext = up[j + 1][0] + go + ge, up[j + 1][1] + ge
        if j > 0:
            i_open, i_ext = S[r][j - 1][0] + go + ge, S[r][j - 1][1] + ge
        dele, ins = max(d_open, d_ext), max(i_open, i_ext)
        assert max(dele, ins) == S[r][j][1]
        out["ties_insdel"] += int(ins == dele)
        if ins > dele:
            ops.append(("I", t))
            start = t
            out["n_ins"] += 1
            out["ties_open"] += int(i_ext == i_open)
            gap = i_ext > i_open
            j -= 1
        else:
            ops.append(("D", r))
            out["n_del"] += 1
            out["ties_open"] += int(d_ext == d_open)
            gap = d_ext > d_open
            r, j = r - 1, j + 1
    ops.reverse()
    out["ops"], out["start_idx"] = ops, start
    pending = 0
    for op in ops:
        if op[0] == "I":
            pending += 1
        else:
            out["col_idx"][op[1]] = op[2] if op[0] == "M" else DELETED
            out["col_ins"][op[1]] = pending
            pending = 0
    out["tail_ins"] = pending
    return out


def rescore(res, flank, sequence, p, cons):
    """The path's score without any DP: matrix[cons[r]][base] over matched columns, go + len * ge per maximal run of gap
    moves, no go for a run that begins at the origin cell (its gap state is 0, ram_extend.c:942-943)."""
    mat = np.ascontiguousarray(p.matrix, np.int64)
    total, in_run = 0, False
    for k, op in enumerate(res["ops"]):
        if op[0] == "M":
            total += int(mat[int(cons[op[1]]) * 100 + flank.base(op[2], sequence)])
            in_run = False
        else:
            if not in_run and not (k == 0 and res["origin"]):
                total += p.gapopen
            total += p.gapextn
            in_run = True
    return total


def consumed_is_contiguous(res):
    """Consumed positions run from start_idx to end_idx without a hole."""
    ts = [op[-1] for op in res["ops"] if op[0] != "D"]
    return ts == list(range(res["start_idx"], res["end_idx"] + 1))


def walk_family(direction, cores, sequence, p, cons):
    """Every extendable core of the direction, in flank order: (core indices, list of walk() results)."""
    ext = cores.right_ext if direction else cores.left_ext
    idx = [n for n in range(cores.n) if ext[n]]
    return idx, [walk(direction, cores, n, sequence, p, cons) for n in idx]


# ---------------------------------------------------------------------------------------------------- -outaln text

def _char(code):
    return "ACGTacgt"[code] if 0 <= code < 8 else "N"


def body(res, flank, sequence, rows, direction):
    """One record's body: `rows` column characters (upper-case base, '-' for a deleted column and above end_row), lower-case
    inserted bases where they fall; a left extension reads reversed."""
    out, col = [], 0
    for op in res["ops"]:
        if op[0] == "I":
            out.append(_char(flank.base(op[1], sequence)).lower())
        elif op[0] == "M":
            out.append(_char(flank.base(op[2], sequence)).upper())
            col += 1
        else:
            out.append("-")
            col += 1
    assert col == res["end_row"] + 1
    out.append("-" * (rows - col))
    s = "".join(out)
    return s if direction else s[::-1]


def render_block(direction, cons, names, core_idx, results, cores, sequence, W):
    """The block of one direction: header, kept consensus, one record per extendable core in flank order."""
    rows = len(cons)
    c = "".join("ACGT"[int(b)] for b in cons)
    lines = [f">{'right' if direction else 'left'}-extension {rows} bp", c if direction else c[::-1]]
    for n, res in zip(core_idx, results):
        lines.append(f">{names[n]}  dir={'right' if direction else 'left'},end_row={res['end_row']},start={res['start_idx']},"
                     f"end={res['end_idx']},score={res['score']}")
        lines.append(body(res, Flank(direction, cores, n, W), sequence, rows, direction))
    return "\n".join(lines) + "\n"


def parse_outaln(text):
    """-> {"right": (ret, consensus, [(name, meta dict, body)]), "left": ...}"""
    lines = text.splitlines()
    out, cur, k = {}, None, 0
    while k < len(lines):
        head, seq = lines[k], lines[k + 1]
        k += 2
        assert head.startswith(">")
        if head.startswith(">right-extension ") or head.startswith(">left-extension "):
            cur = head[1:].split("-")[0]
            out[cur] = (int(head.split()[1]), seq, [])
        else:
            name, meta = head[1:].split("  ")
            out[cur][2].append((name, dict(kv.split("=") for kv in meta.split(",")), seq))
    return out


def overlap_avoidance(fs):
    """The reference's double loop between the two directions (ram_extend.c:445-499) on a loaded FlankSet: a core's bound is
    pulled in to where another core's right extension ends.  Changes fs.cores.lower / upper in place."""
    c = fs.cores
    n = c.n
    seq_lo = lambda s: 0 if s == 0 else int(fs.boundaries[s - 1])
    for s in range(n):
        si = int(c.seq_idx[s])
        ext = int(c.right_pos[s]) - int(c.right_len[s]) if c.orient[s] else int(c.right_pos[s]) + int(c.right_len[s])
        g = int(fs.offsets[si]) + (ext - seq_lo(si) + 1)
        for r in range(n):
            ri = int(c.seq_idx[r])
            if fs.identifiers[si] == fs.identifiers[ri] and g > int(fs.offsets[ri]):
                pos = seq_lo(ri) + (g - int(fs.offsets[ri]))
                if c.orient[r]:
                    if int(c.left_pos[r]) <= pos <= int(c.upper[r]):
                        c.upper[r] = pos
                else:
                    if int(c.lower[r]) <= pos <= int(c.left_pos[r]):
                        c.lower[r] = pos
