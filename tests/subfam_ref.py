"""Reference side of the split of an extension's copies into subfamilies (a helper, not a test): the contract of include/ramx.h
(ramx_link_components, ramx_dev_subfamilies) restated on the bit sets of linkage_ref.planes_of, and the renderer of the
`-outsubfam` text.

A plane is a Python integer used as a bit set (bit i: flank i of the family).  The set of copies that disagree with pattern k at
variant v is cover & (plane ^ (everyone if pat_k[v] else nobody)); a copy's distance is the number of such sets it is in, its
label the first smallest, a count the popcount of plane & group.  Nothing here reads device output."""
import numpy as np

from repeatafterme_amd.datamodel import PLANE_COVER, PLANE_NAMES

import linkage_ref as lr

SUBFAM_MAX = 8


def variants_of(planes):
    """-> (index in the list of every variant, index of its row's cover plane or None)"""
    where = {(int(x["row"]), int(x["cls"])): k for k, x in enumerate(planes)}
    var = [k for k, x in enumerate(planes) if int(x["cls"]) != PLANE_COVER]
    return var, [where.get((int(planes[k]["row"]), PLANE_COVER)) for k in var]


def components(planes, links, K):
    """links: (p, q) pairs of indices into planes -> (init uint8 [V][K'], component int32 [V]); K' = 1 + kept components"""
    var, _ = variants_of(planes)
    num = {p: v for v, p in enumerate(var)}
    V = len(var)
    adj = {v: set() for v in range(V)}
    for p, q in links:
        adj[num[p]].add(num[q])
        adj[num[q]].add(num[p])
    seen, comps = set(), []
    for v in range(V):
        if v in seen:
            continue
        todo, comp = [v], set()
        while todo:
            a = todo.pop()
            if a not in comp:
                comp.add(a)
                todo.extend(adj[a])
        seen |= comp
        if len(comp) >= 2:
            comps.append(sorted(comp))
    comps = sorted(comps, key=lambda c: (-len(c), c[0]))[:K - 1]
    init = np.zeros((V, len(comps) + 1), np.uint8)
    which = np.zeros(V, np.int32)
    for j, c in enumerate(comps):
        init[c, j + 1] = 1
        which[c] = j + 1
    return init, which


def bits_of(s, n):
    """bit set -> bool [n]"""
    return np.unpackbits(np.frombuffer(s.to_bytes((n + 7) // 8 or 1, "little"), np.uint8), bitorder="little")[:n].astype(bool)


def distances(pl, planes, pats, n):
    """pats uint8 [V][K] -> int32 [n][K]"""
    var, cov = variants_of(planes)
    sets = [pl[(int(x["row"]), int(x["cls"]))] for x in planes]
    everyone = (1 << n) - 1
    K = pats.shape[1]
    d = np.zeros((n, K), np.int32)
    for v, (p, c) in enumerate(zip(var, cov)):
        for k in range(K):
            d[:, k] += bits_of(sets[c] & (sets[p] ^ (everyone if pats[v, k] else 0)), n)
    return d


def assign(d):
    """int32 [n][K] -> labels: the first smallest"""
    return np.array([min(range(d.shape[1]), key=lambda k: (row[k], k)) for row in d], np.int32).reshape(-1)


def groups(labels, K):
    """-> the K groups as bit sets"""
    g = [0] * K
    for i, k in enumerate(labels):
        g[int(k)] |= 1 << i
    return g


def counts(pl, planes, labels, K):
    """-> (cnt int32 [K][P], size int32 [K])"""
    g = groups(labels, K)
    sets = [pl[(int(x["row"]), int(x["cls"]))] for x in planes]
    cnt = np.array([[bin(s & m).count("1") for s in sets] for m in g], np.int32).reshape(K, len(sets))
    return cnt, np.array([bin(m).count("1") for m in g], np.int32)


def update(planes, pats, cnt, size):
    var, cov = variants_of(planes)
    new = pats.copy()
    for k in range(pats.shape[1]):
        if size[k] == 0:
            continue                                            # an empty group keeps its pattern
        for v, (p, c) in enumerate(zip(var, cov)):
            new[v, k] = 1 if 2 * int(cnt[k, p]) > int(cnt[k, c]) else 0     # exactly half is not a majority
    return new


def mask_words(labels, K):
    n = len(labels)
    T = (n + 63) // 64
    out = np.zeros((K, T), np.uint64)
    for k, m in enumerate(groups(labels, K)):
        for t in range(T):
            out[k, t] = (m >> (64 * t)) & (2 ** 64 - 1)
    return out


def iterate(pl, planes, init, n, max_iter=8):
    """The iteration of ramx_dev_subfamilies on one family of n flanks -> dict(labels, masks, cnt, size, patterns, dist,
    iterations, converged)."""
    init = np.asarray(init, np.uint8)
    K = init.shape[1] if init.ndim == 2 else 1              # no variant: [0][K]
    pats = init.reshape(len(variants_of(planes)[0]), K).copy()
    assert 1 <= K <= SUBFAM_MAX and max_iter >= 1 and None not in variants_of(planes)[1]
    labels, it = None, 0
    while True:
        d = distances(pl, planes, pats, n)
        new = assign(d)
        it += 1
        stable = K == 1 or (labels is not None and np.array_equal(new, labels))
        labels = new
        cnt, size = counts(pl, planes, labels, K)
        if stable or it == max_iter:
            return dict(labels=labels, masks=mask_words(labels, K), cnt=cnt, size=size, patterns=pats, dist=d, iterations=it,
                        converged=int(stable))
        pats = update(planes, pats, cnt, size)


def list_with(rows, V, first_row=0):
    """The first V variants (cls != 6, all seven classes a row) from first_row on, with their rows' cover planes, as a list."""
    var = [(r, c) for r in range(first_row, rows) for c in range(lr.CLASSES) if c != PLANE_COVER][:V]
    assert len(var) == V
    return lr.as_planes(sorted(set(var) | {(r, PLANE_COVER) for r, _ in var}))


def random_init(V, K, seed):
    """Pattern 0 empty, the others one bit in three."""
    init = (np.random.default_rng(seed).integers(0, 3, (V, K)) == 0).astype(np.uint8)
    init[:, 0] = 0
    return init


def copy_init(pl, planes, K, n, seed):
    """Pattern 0 empty, the others what K - 1 copies of the family carry themselves (copies drawn with `seed`): patterns that are
    near some copies, as the linked components are, for lists no component was computed for."""
    var, _ = variants_of(planes)
    init = np.zeros((len(var), K), np.uint8)
    pick = np.random.default_rng(seed).choice(n, size=min(K - 1, n), replace=False)
    for k, i in enumerate(pick):
        init[:, k + 1] = [pl[(int(planes[p]["row"]), int(planes[p]["cls"]))] >> int(i) & 1 for p in var]
    return init


# ---------------------------------------------------------------------------------------------------- -outsubfam text

def pattern_text(planes, pats, k):
    var, _ = variants_of(planes)
    on = [f"{int(planes[p]['row'])}:{PLANE_NAMES[int(planes[p]['cls'])]}" for v, p in enumerate(var) if pats[v, k]]
    return ",".join(on) if on else "-"


SUBFAM_HEADER = ("#group\tdir\tgroup\tsize\titerations\tconverged\tpattern\trefined_bp\treplays\trefined_converged\tconsensus\n"
                 "#copy\tdir\tcopy\tlabel\tdistances\n")


def render_block(direction, names, core_idx, planes, res, refined):
    """res: what iterate() returns; refined: {group: (refined consensus in row order, replays, converged)} for the kept groups"""
    tag = "right" if direction else "left"
    K = res["patterns"].shape[1] if res["patterns"].ndim == 2 and res["patterns"].shape[0] else len(res["size"])
    lines = []
    for k in range(K):
        head = ["group", tag, str(k), str(int(res["size"][k])), str(res["iterations"]), str(res["converged"]),
                pattern_text(planes, res["patterns"], k)]
        if k in refined:
            cons, replays, conv = refined[k]
            seq = "".join("ACGT"[int(b)] for b in (cons if direction else cons[::-1]))
            head += [str(len(cons)), str(replays), str(conv), seq or "-"]
        else:
            head += ["NA", "NA", "NA", "-"]
        lines.append("\t".join(head))
        for i, n in enumerate(core_idx):
            if int(res["labels"][i]) == k:
                lines.append("\t".join(["copy", tag, names[n], str(k)] + [str(int(x)) for x in res["dist"][i]]))
    return "".join(line + "\n" for line in lines)


def render_subfam(blocks):
    """blocks: {1: (names, core_idx, planes, res, refined), 0: ...} -> the file: header, the right block, the left block."""
    return SUBFAM_HEADER + "".join(render_block(d, *blocks[d]) for d in (1, 0) if d in blocks)
