"""numpy restatement of epsilon-lexicase selection (include/evogp_hip.h evogp_hip_lexicase_select, csrc/lexicase.hip,
evogp_amd/algorithm/selection.py): the counter words, the case permutation perm_k, the pick word_k, the down-sampled rows, eps, the
clone classes (exact key-row equality) and the events, one function per event so that any single event can be checked on its own."""
import numpy as np

M64 = (1 << 64) - 1
ROW_FEISTEL = 2**21          # + r, r < 4: round keys of event k
ROW_PICK = 2**21 + 4
ROW_SAMPLE = 2**21 + 5


def mix64(x):
    """splitmix64's finaliser on uint64 arrays (wrap-around)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def counter_base(seed, generation):
    return int(mix64(np.array([(seed * 1000003 + generation) & M64], dtype=np.uint64))[0])


def counter_words(seed, generation, row, items):
    """word `row` of the given items (uint64 array): values in [0, 2^31 - 1)"""
    base = counter_base(seed, generation)
    items = np.asarray(items, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = mix64(np.uint64((base + (row << 40)) & M64) + items)
    return ((x >> np.uint64(33)) & np.uint64(0x7FFFFFFF)) % np.uint64(0x7FFFFFFF)


def half_width(n):
    b = 0
    while (1 << b) < n:
        b += 1
    return (b + (b & 1)) // 2


def perm(seed, generation, k, n, positions=None):
    """perm_k(j) for the given positions (default: all of [0, n)) -- int64 array"""
    j = np.arange(n, dtype=np.uint64) if positions is None else np.asarray(positions, dtype=np.uint64)
    if n <= 1:
        return np.zeros(j.shape, dtype=np.int64)
    h = half_width(n)
    mask = np.uint64((1 << h) - 1)
    rk = [np.uint64(int(counter_words(seed, generation, ROW_FEISTEL + r, [k])[0])) for r in range(4)]

    def feistel(x):
        L, R = x >> np.uint64(h), x & mask
        for r in range(4):
            f = (mix64((rk[r] << np.uint64(32)) | R) >> np.uint64(32)) & mask
            L, R = R, L ^ f
        return (L << np.uint64(h)) | R

    x = feistel(j)
    while True:
        out = x >= np.uint64(n)
        if not out.any():
            return x.astype(np.int64)
        x[out] = feistel(x[out])


def pick_word(seed, generation, k):
    return int(counter_words(seed, generation, ROW_PICK, [k])[0])


def sample_rows(seed, generation, D, rate):
    """the down-sampled rows of a call: the m = max(1, round(rate D)) rows of smallest word (ties: lower row), ascending; None = all"""
    m = max(1, round(rate * D))
    if m >= D:
        return None
    w = counter_words(seed, generation, ROW_SAMPLE, np.arange(D)).astype(np.int64)
    return np.sort(np.argsort(w, kind="stable")[:m])


def case_errors(pred, y, use_mse):
    """errors[d][t] (case-major) from batch_forward outputs pred (pop, D, out) and labels y (D, out), in float32, o ascending"""
    pred = np.asarray(pred, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    s = np.zeros(pred.shape[:2], dtype=np.float32)
    with np.errstate(all="ignore"):
        for o in range(pred.shape[2]):
            diff = pred[:, :, o] - y[None, :, o]
            s = s + (diff * diff if use_mse else np.abs(diff))
        return (s / np.float32(pred.shape[2])).T.copy()


def lowmed(v):
    v = np.sort(v)
    return v[(len(v) - 1) // 2]


def epsilon(errors):
    """(pop, n) -> (n,) float32: the MAD of every case's finite errors (lower medians), 0 without a finite error"""
    errors = np.asarray(errors, dtype=np.float32)
    out = np.zeros(errors.shape[1], dtype=np.float32)
    for c in range(errors.shape[1]):
        e = errors[:, c][np.isfinite(errors[:, c])]
        if len(e):
            m = lowmed(e)
            with np.errstate(over="ignore"):
                out[c] = lowmed(np.abs(e - m))
    return out


def keys(E):
    """key(x) of case-major errors: NaN -> +inf, -0 -> +0"""
    K = np.array(E, dtype=np.float32, copy=True)
    K[np.isnan(K)] = np.inf
    K[K == 0] = 0.0
    return K


class Classes:
    """clone classes of case-major errors E[n][pop]: exact key-row equality; classes in ascending order of their smallest tree"""

    def __init__(self, E):
        K = keys(E)
        bits = np.ascontiguousarray(K.T).view(np.uint32)                       # (pop, n)
        _, first, inverse = np.unique(bits, axis=0, return_index=True, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        order = np.argsort(first, kind="stable")                               # unique-row id -> rank by smallest tree
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        self.of_tree = rank[inverse]                                           # class id of every tree
        self.rep = first[order]                                                # smallest tree of every class
        self.size = np.bincount(self.of_tree, minlength=len(order))
        self.sorted = np.argsort(self.of_tree, kind="stable")                  # members class by class, ascending within a class
        self.offset = np.concatenate([[0], np.cumsum(self.size)[:-1]])
        self.K = K

    def members(self, c):
        return self.sorted[self.offset[c]: self.offset[c] + self.size[c]]

    def __len__(self):
        return len(self.rep)


def sanitize_eps(eps):
    eps = np.asarray(eps, dtype=np.float32).copy()
    eps[~(eps > 0)] = 0.0
    return eps


def event(E, eps, seed, generation, k, classes=None, return_steps=False):
    """the winner of event k (and the steps after the first case when return_steps)"""
    classes = Classes(E) if classes is None else classes
    K = classes.K
    eps = sanitize_eps(eps)
    n = K.shape[0]
    pool = np.arange(len(classes))
    order = perm(seed, generation, k, n)
    steps = 0
    for j in range(n):
        if len(pool) <= 1:
            break
        steps += j > 0
        c = order[j]
        kv = K[c, classes.rep[pool]]
        m = kv.min()
        with np.errstate(invalid="ignore"):
            thr = np.float32(m) + np.float32(eps[c])
            pool = pool[(kv <= thr) | (kv == m)]
    # L = the members of the pool's classes, class by class: position r of L
    cum = np.cumsum(classes.size[pool])
    r = pick_word(seed, generation, k) % int(cum[-1])
    q = int(np.searchsorted(cum, r, side="right"))
    w = int(classes.members(pool[q])[r - (int(cum[q - 1]) if q else 0)])
    return (w, steps) if return_steps else w


def select(E, eps, n_events, seed, generation, events=None):
    """winners of the given events (default: all n_events) -- int32 array"""
    classes = Classes(E)
    ks = range(n_events) if events is None else events
    return np.array([event(E, eps, seed, generation, k, classes) for k in ks], dtype=np.int32)
