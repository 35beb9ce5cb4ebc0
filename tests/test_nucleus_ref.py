"""tests/nucleus_ref.py on its own (no GPU): the reference's kept set against a brute-force sort
on tiny rows, and the whole sweep of tests/test_select_token_p_gpu.py run on the reference alone,
to hold the sweep to its caps: how many cases the fp32 bands leave ambiguous, how many draws fall
inside an eps band, and how many kept sets are large enough for the filters to matter.

The caps, on the 13608 continuous row cases, and what this generator gives: ambiguous < 1 %
(29 cases, 0.21 %), u inside an eps band < 1 % (4, 0.03 %), kept sets of at least 3 entries
>= 25 % (4386, 32.2 %). The quantised rows tie everywhere and are printed, not capped (205
ambiguous, 1.51 %; 83 inside a band, 0.61 %).
"""
import numpy as np

import nucleus_ref as R


def test_kept_set_equals_brute_force_on_tiny_rows():
    rng = np.random.default_rng(7)
    n = 0
    for V in (1, 2, 3, 5, 8, 13):
        for quantised in (False, True):
            for T in (0.5, 1.0, 2.0):
                x = R.sampling_rows(rng, 4, V, T, quantised)
                for b in range(4):
                    for top_k in (0, 1, 3, V - 1, V):
                        row = R.Row(x[b], T, top_k)
                        for top_p in (1e-6, 0.1, 0.35, 0.5, 0.9, 0.99, 1.0):
                            for min_p in (0.0, 0.02, 0.3, 1.0):
                                want = R.brute_force(x[b], T, top_k, top_p, min_p)
                                got = sorted(row.prefix(row.kept(top_p, min_p)).tolist())
                                assert got == want, (V, quantised, T, b, top_k, top_p, min_p)
                                lo, hi = row.bounds(top_p, min_p)
                                assert 1 <= lo <= len(want) <= hi <= row.k
                                n += 1
    assert n > 5000


def test_hand_made_row():
    """4 entries at 0, 12 at -1, the rest at -3 (V = 64, T = 1), top_p = 0.6: the four maxima and
    the first 7 of the ties by index; min_p = 0.5 keeps the maxima only, 0.3 the ties too."""
    V = 64
    x = np.full(V, -3.0, np.float32)
    top = [5, 20, 41, 63]
    ties = [1, 7, 8, 15, 22, 30, 33, 40, 47, 52, 58, 61]
    x[top] = 0.0
    x[ties] = -1.0
    row = R.Row(x, 1.0, 0)
    assert sorted(row.prefix(row.kept(0.6, 0.0)).tolist()) == sorted(top + ties[:7])
    assert row.bounds(0.6, 0.0) == (11, 11)
    assert sorted(row.prefix(row.kept(1.0, 0.5)).tolist()) == top
    assert sorted(row.prefix(row.kept(1.0, 0.3)).tolist()) == sorted(top + ties)
    assert sorted(row.prefix(row.kept(0.6, 0.5)).tolist()) == top
    # top_k cuts inside the tie class first: K is the maxima and 9 ties (mass 4 + 9 / e = 7.311),
    # and 0.6 of it, 4.387, needs two of them (4 + 1 / e = 4.368 falls short)
    row = R.Row(x, 1.0, 13)
    assert sorted(row.prefix(row.kept(0.6, 0.0)).tolist()) == sorted(top + ties[:2])
    assert R.Row(x, 1.0, 0).kept(1e-6, 0.0) == 1


def test_the_sweep_on_the_reference_alone():
    """Every case of the GPU sweep, judged with the reference's own float64 id: all pass, and the
    shares that say what the sweep can tell stay inside their caps on the continuous rows."""
    tot = {False: dict(n=0, amb=0, band=0, kept3=0), True: dict(n=0, amb=0, band=0, kept3=0)}
    for V, B, T, k, quantised, rows, settings in R.sweep_cases():
        refs = [R.Row(rows[b], T, k) for b in range(B)]
        for top_p, min_p, seed in settings:
            u = R.uniform24_ref(seed, np.arange(B))
            for b in range(B):
                i = refs[b].choose(float(u[b]), top_p, min_p)
                j = refs[b].judge(i, float(u[b]), top_p, min_p)
                assert j["inside"] and j["ok"], (V, B, T, k, quantised, top_p, min_p, b, i)
                t = tot[quantised]
                t["n"] += 1
                t["amb"] += j["ambiguous"]
                t["band"] += j["band"]
                t["kept3"] += j["kept"] >= 3
    for quantised, name in ((False, "continuous"), (True, "quantised")):
        t = tot[quantised]
        print(f"{name}: {t['n']} row cases; ambiguous {t['amb']} ({100 * t['amb'] / t['n']:.2f} %); u inside an "
              f"eps band {t['band']} ({100 * t['band'] / t['n']:.2f} %); kept set >= 3 entries {t['kept3']} "
              f"({100 * t['kept3'] / t['n']:.1f} %)")
    c = tot[False]
    assert c["n"] == 13608
    assert c["amb"] / c["n"] < 0.01
    assert c["band"] / c["n"] < 0.01
    assert c["kept3"] / c["n"] >= 0.25
