"""A NumPy statement of speculative decoding's host-checkable rules (include/minitorch_hip.h,
"speculative decoding"): the prompt-lookup draft rule of mt_spec_draft, steps 2-3 of
mt_spec_accept (given the chosen ids c), and ``simulate``, which replays a row's plain-generation
ids through both and returns the per-step counts speculative decoding must show. Helper module:
the tests that use it are test_spec_ref.py (CPU) and test_spec_*_gpu.py."""
import numpy as np


def draft(tokens, held, k, max_ngram):
    """One row of mt_spec_draft. tokens: the row's S ints. Returns (feed [k + 1], n_draft)."""
    tokens = [int(t) for t in tokens]
    L = min(max(int(held), 1), len(tokens))
    ext = tokens[:L]
    feed = [ext[L - 1]]
    for g in range(min(max_ngram, L - 1), 0, -1):
        tail = ext[L - g:L]
        for s in range(L - g - 1, -1, -1):  # the largest s first
            if ext[s:s + g] == tail:
                for i in range(k):
                    ext.append(ext[s + g + i])
                    feed.append(ext[-1])
                return feed, k
    return feed + [feed[0]] * k, 0


def accept(c, feed, n_draft, count, held, limit, eos=None):
    """Steps 2-3 of mt_spec_accept for one live row, c the k + 1 chosen ids. Returns a dict:
    a (leading drafts that match), written (the ids written to history[count:] and tokens[held:],
    a stopping eos included), count / held after, done, accepted (what the counter grows by)."""
    k = len(c) - 1
    nd = min(max(int(n_draft), 0), k)
    a = 0
    while a < nd and feed[1 + a] == c[a]:
        a += 1
    e = min(a + 1, limit - count)
    written, stopped = [], False
    for j in range(max(e, 0)):
        written.append(int(c[j]))
        if eos is not None and eos >= 0 and c[j] == eos:
            stopped = True
            break
    w = len(written)
    return dict(a=a, written=written, count=count + w, held=held + w,
                done=bool(stopped or count + w >= limit), accepted=max(min(a, w - 1), 0), drafted=nd)


def simulate(ids, prompt, k, ngram, limit, eos=None):
    """The speculative steps of one row whose plain generation returned `ids` from `prompt` under
    the token limit `limit` (a row that returned fewer was stopped by `eos`, which plain generation
    chose next). Exact-match verification makes the chosen ids those of plain generation, so the
    steps are a function of them alone. The first token comes from the prefill (count = 1).
    Returns dict(steps, tokens, drafted, accepted, per_step=[(n_draft, a, written), ...]); tokens
    counts every chosen id, the first and a stopping eos included."""
    stream = [int(t) for t in ids]
    if len(stream) < limit:
        assert eos is not None, "a row shorter than its limit was stopped by an eos"
        stream.append(int(eos))
    if limit <= 0 or not stream:
        return dict(steps=0, tokens=0, drafted=0, accepted=0, per_step=[])
    S = len(prompt) + len(stream) + k + 2
    tokens = np.zeros(S, dtype=np.int64)
    tokens[:len(prompt)] = prompt
    tokens[len(prompt)] = stream[0]
    count, held = 1, len(prompt) + 1
    done = (eos is not None and stream[0] == eos) or count >= limit
    out = dict(steps=0, tokens=1, drafted=0, accepted=0, per_step=[])
    while not done:
        feed, nd = draft(tokens, held, k, ngram)
        # what plain generation chooses after feed[0 .. i]: its next ids while the drafts are right
        # (past the first wrong draft, or past the stream's end, the value is never looked at)
        c = [stream[count + i] if count + i < len(stream) else -1 for i in range(k + 1)]
        r = accept(c, feed, nd, count, held, limit, eos)
        assert all(t >= 0 for t in r["written"])
        tokens[held:held + len(r["written"])] = r["written"]
        count, held, done = r["count"], r["held"], r["done"]
        out["steps"] += 1
        out["tokens"] += len(r["written"])
        out["drafted"] += r["drafted"]
        out["accepted"] += r["accepted"]
        out["per_step"].append((nd, r["a"], len(r["written"])))
    return out


def totals(rows):
    """The call's spec_stats from the rows' simulate() results: the steps while any row was live
    and the sums of the other counters."""
    return dict(steps=max([r["steps"] for r in rows] + [0]), tokens=sum(r["tokens"] for r in rows),
                drafted=sum(r["drafted"] for r in rows), accepted=sum(r["accepted"] for r in rows))
