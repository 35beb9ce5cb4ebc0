"""A float64 NumPy restatement of mt_select_token_p's contract (include/minitorch_hip.h), the
yardstick of tests/test_select_token_p_gpu.py and tests/test_nucleus_generate_gpu.py, and the
sweep both it and tests/test_nucleus_ref.py run.

The kept set K of top_k in the order (fp32 value descending, index ascending), e_i =
exp((x_i - max) / T), N the shortest prefix of K whose mass reaches top_p times K's, M the
entries with e_i >= min_p (a prefix too), the kept set the shorter prefix, the id the first kept
index whose running probability exceeds u.

What an fp32 kernel may differ by, and no more:
  eps = 1e-5 + V 2^-24 on a cumulative probability, the bound of test_select_token_gpu.py taken
  over unchanged (the rounded exponent argument plus an fp32 sum of V terms);
  1e-5 relative on an e_i compared with min_p (the exponent argument is at most 32 in magnitude
  and carries two fp32 roundings, 32 * 2^-23 = 3.8e-6, plus expf's own error).
So the nucleus may be any prefix length from n_lo (at top_p - eps) to n_hi (at top_p + eps), the
min_p prefix any from m_lo to m_hi, and an id passes when it lies in the prefix of length
min(n_hi, m_hi) and meets the CDF bound of test_select_token_gpu.py for some kept length in
[max(1, min(n_lo, m_lo)), min(n_hi, m_hi)]. A case with more than one such length is ambiguous.
"""
import numpy as np

from train_kernels_ref import uniform24_ref  # noqa: F401  (the uniform of (seed, b))

VS = (1, 63, 64, 65, 97, 1025, 4099)
BS = (1, 3, 17)
TEMPS = (0.5, 1.0, 2.0)
MIN_PS = (0.0, 0.02, 0.3)
E_BAND = 1e-5


def top_ks(V):
    return (0, 5, V - 1)


def top_ps(V):
    # at V >= 1025 eps is as wide as a tail token's mass: 0.9 and 0.99 would mostly be ambiguous
    return (0.1, 0.5, 0.9, 0.99) if V <= 97 else (0.1, 0.5)


def eps_of(V):
    return 1e-5 + V * 2.0 ** -24


def sampling_rows(rng, B, V, T, quantised):
    """|logit / T| <= 16: y in [-16, 16] times the fp32 T. Continuous rows are 3 N(0, 1) clipped
    (flat enough that a nucleus holds several tokens), quantised ones 8 levels (ties everywhere)."""
    if quantised:
        y = rng.integers(0, 8, (B, V)) * 4.0 - 14.0
    else:
        y = np.clip(3.0 * rng.standard_normal((B, V)), -16.0, 16.0)
    return (y.astype(np.float32) * np.float32(T)).astype(np.float32)


def sweep_cases():
    """(V, B, T, top_k, quantised, rows, [(top_p, min_p, seed), ...]) from one generator: the rows
    of a (V, B, T, top_k, quantised) are shared by its top_p / min_p settings, each with a seed of
    its own."""
    rng = np.random.default_rng(2025)
    n = 0
    for V in VS:
        for B in BS:
            for T in TEMPS:
                for k in top_ks(V):
                    for quantised in (False, True):
                        rows = sampling_rows(rng, B, V, T, quantised)
                        settings = []
                        for top_p in top_ps(V):
                            for min_p in MIN_PS:
                                n += 1
                                settings.append((top_p, min_p, 1000003 * n + 17))
                        yield V, B, T, k, quantised, rows, settings


class Row:
    """One fp32 row under (T, top_k): K's order and the float64 e_i and running mass along it."""

    def __init__(self, x, T, top_k):
        x = np.asarray(x, dtype=np.float32)
        V = x.size
        k = V if (top_k <= 0 or top_k >= V) else int(top_k)
        order = np.lexsort((np.arange(V), -x.astype(np.float64)))  # value descending, index ascending
        self.V, self.k = V, k
        self.order = order[:k]
        xs = x[self.order].astype(np.float64)
        self.e = np.exp((xs - xs[0]) / float(np.float32(T)))
        self.mass = np.cumsum(self.e)
        self.eps = eps_of(V)

    def nucleus(self, top_p):
        """The shortest prefix length whose mass reaches top_p of K's; at least 1, at most k."""
        if top_p >= 1.0:
            return self.k
        if top_p <= 0.0:
            return 1
        n = int(np.searchsorted(self.mass, top_p * self.mass[-1], side="left")) + 1
        return min(max(n, 1), self.k)

    def floor(self, min_p):
        """The number of entries with e_i >= min_p (a prefix: e falls along K's order)."""
        if min_p <= 0.0:
            return self.k
        return int(np.count_nonzero(self.e >= min_p))

    def kept(self, top_p, min_p):
        """The contract's kept length at exactly (top_p, min_p)."""
        return max(1, min(self.nucleus(top_p), self.floor(float(np.float32(min_p)))))

    def bounds(self, top_p, min_p):
        """(lo, hi): the kept lengths an fp32 implementation may arrive at."""
        if top_p >= 1.0:
            n_lo = n_hi = self.k
        else:
            n_lo, n_hi = self.nucleus(top_p - self.eps), self.nucleus(top_p + self.eps)
        mp = float(np.float32(min_p))
        m_lo, m_hi = self.floor(mp * (1 + E_BAND)), self.floor(mp * (1 - E_BAND))
        return max(1, min(n_lo, m_lo)), max(1, min(n_hi, m_hi))

    def prefix(self, length):
        return self.order[:length]

    def cdf(self, length):
        """(kept indices ascending, float64 CDF over them) of the prefix of that length."""
        pos = np.sort(self.order[:length])
        # e by index: order[:length] sorted by index, their e alongside
        by_index = np.argsort(self.order[:length], kind="stable")
        p = self.e[:length][by_index]
        return pos, np.cumsum(p / p.sum())

    def choose(self, u, top_p, min_p):
        """The contract's id in float64: the first kept index whose running probability exceeds u."""
        pos, cdf = self.cdf(self.kept(top_p, min_p))
        return int(pos[min(int(np.searchsorted(cdf, u, side="right")), pos.size - 1)])

    def judge(self, i, u, top_p, min_p):
        """dict(inside: i lies in the widest allowed prefix; ok: and meets the CDF bound for some
        allowed kept length; ambiguous: more than one length is allowed; band: u within eps of an
        inner CDF boundary of the contract's own kept set; kept: that set's size)."""
        lo, hi = self.bounds(top_p, min_p)
        inside = bool(np.any(self.order[:hi] == i))
        ok = False
        if inside:
            for length in range(lo, hi + 1):
                pos, cdf = self.cdf(length)
                j = int(np.searchsorted(pos, i))
                if j < pos.size and pos[j] == i:
                    below = cdf[j - 1] if j else 0.0
                    if below - self.eps <= u < cdf[j] + self.eps:
                        ok = True
                        break
        n0 = self.kept(top_p, min_p)
        _, cdf0 = self.cdf(n0)
        band = bool(cdf0.size > 1 and np.abs(cdf0[:-1] - u).min() < self.eps)
        return dict(inside=inside, ok=ok, ambiguous=hi > lo, band=band, kept=n0)


def brute_force(x, T, top_k, top_p, min_p):
    """The contract's kept set of one row, by a plain Python sort and loop (no searchsorted, no
    cumsum): the indices, ascending."""
    x = [float(v) for v in np.asarray(x, dtype=np.float32)]
    V = len(x)
    k = V if (top_k <= 0 or top_k >= V) else top_k
    order = sorted(range(V), key=lambda i: (-x[i], i))[:k]
    T = float(np.float32(T))
    e = [float(np.exp((x[i] - x[order[0]]) / T)) for i in order]
    total = 0.0
    for v in e:  # the same left-to-right float64 sum np.cumsum forms
        total += v
    n = k
    if top_p < 1.0:
        run, n = 0.0, 0
        for v in e:
            run += v
            n += 1
            if run >= top_p * total:
                break
    mp = float(np.float32(min_p))
    m = sum(1 for v in e if v >= mp) if mp > 0.0 else k
    return sorted(order[:max(1, min(n, m))])
