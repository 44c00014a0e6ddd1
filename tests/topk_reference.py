"""Host side of the df3d_topk_keys tests (numpy only): the oracle, a restatement of which path of csrc/topk.hip an input
takes, and the key families that drive every path.

`select` is the oracle: a row-wise np.sort.  `branch` / `trace` restate the DECISIONS of topk.hip -- the two 4096-bin
thresholds of the histogram kernels, the counts A (below the 24-bit threshold prefix) and P (tied with it) of the compaction,
and the levels of the in-workgroup radix of topk_final_kernel with their exit test -- so that a test can state which path an
input is built for.  They describe the intended algorithm (the tie group is the set of keys whose CLAMPED prefix equals the
threshold, the prefix the compaction used); they never produce an expected output."""
import numpy as np

# ---- the constants of csrc/topk.hip, with the lines they mirror
BINS = 4096                       # :39  TK_BINS, bins of every histogram level
TIE_CAP = 4096                    # :40  TK_TIE_CAP, region 1; :233 `P <= TK_TIE_CAP` chooses the region sort
BUF = 8192                        # :41  TK_BUF, the LDS sort buffer; :287 `A + below + P3 <= TK_BUF` ends the radix levels
PREFIX_SHIFT = 30                 # :46  tk_prefix24: (key & low56) >> 30 ...
PREFIX_CLAMP = 0xFFFFFF           # :47  ... clamped to 24 bits
CLAMP_SHIFTS = (54, 42, 30)       # :260 levels -3, -2, -1: only for the clamp prefix, they never end the radix (:287 `level >= 0`)
LEVEL_SHIFTS = (18, 6, 0)         # :260 levels 0, 1, 2
MAX_K = 4096                      # :40  K <= TK_TIE_CAP
MAX_N = 2 ** 31 - 1               # :43  TK_MAX_N
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW56 = np.uint64(0x00FFFFFFFFFFFFFF)
PATHS = ("region", "level0", "level1", "level2", "stream")


def select(keys, k):
    """keys u64 [S, n] -> (out u64 [S, k], count [S]): the k smallest keys of every row in ascending order, the all-ones key
    (masked) last, padded with it where the row has fewer than k keys; count = entries of out that are not all-ones."""
    keys = np.asarray(keys, dtype=np.uint64)
    assert keys.ndim == 2 and k >= 1
    out = np.sort(keys, axis=1)[:, :k]
    if out.shape[1] < k:
        out = np.concatenate([out, np.full((keys.shape[0], k - out.shape[1]), ONES, np.uint64)], axis=1)
    return out, (out != ONES).sum(axis=1)


def _threshold(hist, need):
    """tk_find_threshold: the smallest bin whose inclusive cumulative count reaches `need` (the last bin if none does), and
    the count below that bin"""
    c = np.cumsum(hist)
    T = int(np.searchsorted(c, need, side="left"))
    if T >= len(hist):
        T = len(hist) - 1
    return T, int(c[T] - hist[T])


def trace(keys_row, k):
    """-> dict(path, A, P, fill): the path topk_final_kernel takes for this segment, the region counts of the compaction, and
    (radix paths) the number of keys the exit test compared with the buffer at the level it ended on (stream: at level 2)."""
    row = np.asarray(keys_row, dtype=np.uint64).ravel()
    low = row[row != ONES] & LOW56
    p = np.minimum(low >> np.uint64(PREFIX_SHIFT), np.uint64(PREFIX_CLAMP)).astype(np.int64)
    T1, A1 = _threshold(np.bincount(p >> 12, minlength=BINS), k)
    T2, _ = _threshold(np.bincount(p[(p >> 12) == T1] & 0xFFF, minlength=BINS), k - A1)
    thr24 = (T1 << 12) | T2
    A, P = int((p < thr24).sum()), int((p == thr24).sum())
    if P <= TIE_CAP:
        return dict(path="region", A=A, P=P, fill=A + P)
    members = low[p == thr24]                       # the tie group: by the clamped prefix, like the compaction
    clamp = thr24 == PREFIX_CLAMP
    levels = ([(-3 + i, sh) for i, sh in enumerate(CLAMP_SHIFTS)] if clamp else []) + list(enumerate(LEVEL_SHIFTS))
    chain, sh_prev, below, fill = (0 if clamp else thr24 << PREFIX_SHIFT), (56 if clamp else PREFIX_SHIFT), 0, 0
    for level, sh in levels:
        inside = members[(members >> np.uint64(sh_prev)) == np.uint64(chain >> sh_prev)]
        bins = ((inside >> np.uint64(sh)) & np.uint64((1 << (sh_prev - sh)) - 1)).astype(np.int64)
        hist = np.bincount(bins, minlength=BINS)
        T3, A3 = _threshold(hist, k - A - below)
        chain |= T3 << sh
        below += A3
        sh_prev = sh
        fill = A + below + int(hist[T3])
        if level >= 0 and fill <= BUF:
            return dict(path="level%d" % level, A=A, P=P, fill=fill)
    return dict(path="stream", A=A, P=P, fill=fill)


def branch(keys_row, k):
    return trace(keys_row, k)["path"]


# ---- key families: one shuffled segment each.  base = seg << 56 | hi << 54 | PREFIX << 30; `tie` keys share bits [55:30] with
# base, `below` keys have the same hi and a smaller prefix (strictly below the tie group, so A > 0 at hi = 0), `masked` are all-ones
PREFIX = 0x2A5F31
TIE_KINDS = {                      # name -> (default n, low 30 bits of the tie keys)
    "ties_l0": (6037, lambda rs, m: (rs.randint(0, 4096, size=m).astype(np.uint64) << np.uint64(18)) | np.arange(m, dtype=np.uint64)),
    "ties_l1": (9001, lambda rs, m: np.arange(m, dtype=np.uint64)),
    "ties_l2": (9001, lambda rs, m: np.arange(m, dtype=np.uint64) % np.uint64(64)),        # duplicate keys: legal
    "identical": (9001, lambda rs, m: np.zeros(m, np.uint64)),
    "identical_long": (20011, lambda rs, m: np.zeros(m, np.uint64)),                       # the streaming buffer is re-sorted several times
}
INTENDED = {"ties_l0": "level0", "ties_l1": "level1", "ties_l2": "level2", "identical": "stream", "identical_long": "stream"}
HI_SEG = {0: 0x00, 1: 0x5A, 3: 0xFF}              # the segment byte the tests pair with each hi (0xFF: negative as int64)


def family(name, hi=0, seed=0, tie=None, below=37, masked=29, seg=None):
    """[n] u64, n = tie + below + masked; tie defaults to what makes n the family's default size"""
    n_default, low30 = TIE_KINDS[name]
    tie = n_default - below - masked if tie is None else tie
    seg = HI_SEG[hi] if seg is None else seg
    assert PREFIX - below >= 0 and tie >= 0
    rs = np.random.RandomState(seed * 7919 + hi)
    top = (np.uint64(seg) << np.uint64(56)) | (np.uint64(hi) << np.uint64(54))
    ties = top | (np.uint64(PREFIX) << np.uint64(30)) | low30(rs, tie)
    pre = np.uint64(PREFIX - 1) - np.arange(below, dtype=np.uint64)
    lows = top | (pre << np.uint64(30)) | rs.randint(0, 1 << 30, size=below).astype(np.uint64)
    row = np.concatenate([ties, lows, np.full(masked, ONES, np.uint64)])
    return row[rs.permutation(len(row))]


# capacity edges: name -> (row builder(hi), k, the path at hi = 0).  The pairs sit on the two sides of one comparison.
EDGES = {
    # :233 P <= TK_TIE_CAP.  P is the count of the threshold's CLAMPED prefix: for hi != 0 the 37 keys below sit in that bin too
    "P_4096": (lambda hi: family("ties_l1", hi, 1, tie=TIE_CAP - (37 if hi else 0)), 100, "region"),
    "P_4097": (lambda hi: family("ties_l1", hi, 1, tie=TIE_CAP + 1 - (37 if hi else 0)), 100, "level0"),
    "fill_8192": (lambda hi: family("identical", hi, 2, tie=BUF - 37), 100, "level0"),       # :287 A + below + P3 <= TK_BUF
    "fill_8193": (lambda hi: family("identical", hi, 2, tie=BUF - 37 + 1), 100, "stream"),
    "k4096_A4095": (lambda hi: family("ties_l1", hi, 3, tie=5003, below=4095), 4096, "level1"),   # one key comes from the tie group
}


def small_rows():
    """name -> (row, k): the degenerate sizes"""
    few = family("ties_l1", 0, 4, tie=40, below=5, masked=3)
    return {"k_1": (family("ties_l1", 0, 5), 1), "k_1_ties": (family("ties_l1", 0, 5, below=0), 1),
            "n_1": (few[few != ONES][:1].copy(), 5), "n_below_k": (few, 100),
            "all_masked": (np.full(777, ONES, np.uint64), 60)}


def stack(rows):
    """rows of different lengths -> [S, max n], the shorter ones padded with masked keys"""
    n = max(len(r) for r in rows)
    return np.stack([np.concatenate([r, np.full(n - len(r), ONES, np.uint64)]) for r in rows])
