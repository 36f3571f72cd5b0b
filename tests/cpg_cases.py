"""A family with planted, mostly deaminated CpG sites (a helper, not a test): what the CpG-aware re-call exists for.

planted_family builds a FlankSet laid out as repeatafterme_amd.synth.synth_family's (one window per copy: left flank, core,
right flank; minus-strand copies reverse-complemented).  Both ancestors carry N_SITES `CG` in reading order, at least 6 columns
apart.  In every copy each strand of every planted site deaminates on its own with probability D (C -> T, G -> A, in reading
order) BEFORE the usual divergence (80% substitutions, 10% deletions, 10% insertions of DIV) is applied."""
import numpy as np

from repeatafterme_amd.datamodel import CoreSet, FlankSet

A, C, G, T = 0, 1, 2, 3

N_COPIES, K, L, W, MATRIX = 96, 120, 150, 14, "14p43g"
N_SITES, FIRST, STEP = 8, 9, 14           # reading-order columns of the C of every site: FIRST + STEP * k (its G follows)
D, DIV, MINUS = 0.6, 0.14, 0.4
SEED = 5


def site_columns():
    return [FIRST + STEP * k for k in range(N_SITES)]


def _ancestor(rng):
    anc = rng.integers(0, 4, size=K, dtype=np.int8)
    for c in site_columns():
        anc[c], anc[c + 1] = C, G
    return anc


def _diverged(rng, anc):
    """One copy of an ancestor, in reading order: every planted strand deaminated with probability D, then diverged."""
    v = anc.copy()
    for c in site_columns():
        if rng.random() < D:
            v[c] = T
        if rng.random() < D:
            v[c + 1] = A
    out = []
    for b in v:
        u = rng.random()
        if u < 0.8 * DIV:
            out.append((int(b) + int(rng.integers(1, 4))) & 3)
        elif u < 0.9 * DIV:
            continue
        elif u < DIV:
            out.extend((int(b), int(rng.integers(0, 4))))
        else:
            out.append(int(b))
    return np.asarray(out, np.int8)


def planted_family(seed=SEED, n=N_COPIES, core_len=10, pad=20):
    """-> (FlankSet, right ancestor, left ancestor); both ancestors in reading order: the right one begins at the core, the left
    one ends at it (its column K - 1 touches the core, so row r of the left extension is its column K - 1 - r)."""
    rng = np.random.default_rng(seed)
    anc_r, anc_l = _ancestor(rng), _ancestor(rng)
    core = rng.integers(0, 4, size=core_len, dtype=np.int8)
    F = L + W + pad
    win = 2 * F + core_len
    seq = np.empty((n, win), np.int8)
    minus = rng.random(n) < MINUS
    for i in range(n):
        fill = rng.integers(0, 4, size=2 * F, dtype=np.int8)
        seq[i, :F] = np.concatenate((fill[:F], _diverged(rng, anc_l)))[-F:]
        seq[i, F:F + core_len] = core
        seq[i, F + core_len:] = np.concatenate((_diverged(rng, anc_r), fill[F:]))[:F]
        if minus[i]:
            seq[i] = 3 - seq[i, ::-1]
    off = np.arange(n, dtype=np.int64) * win
    lo_core = off + F                                  # both flanks have F columns: the core begins at F on either strand
    hi_core = lo_core + core_len - 1
    cores = CoreSet(left_pos=np.where(minus, hi_core, lo_core), right_pos=np.where(minus, lo_core, hi_core), lower=off,
                    upper=off + win - 1, orient=minus.astype(np.int8), left_ext=np.ones(n, np.int8), right_ext=np.ones(n, np.int8))
    boundaries = np.concatenate((off[1:], [n * win], [0])).astype(np.uint64)
    return FlankSet(sequence=seq.reshape(-1), boundaries=boundaries, cores=cores), anc_r, anc_l


def sites_in_rows(direction):
    """The planted sites as row pairs (r, r + 1) of the direction's consensus, absent indels in it: for the right extension the C
    is in row r, for the left one (rows run outward from the core) the G is."""
    return [c if direction else K - 2 - c for c in site_columns()]
