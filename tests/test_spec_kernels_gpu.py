"""mt_spec_draft and mt_spec_accept on the GPU against tests/spec_ref.py (integer equality
throughout). The chosen ids c_i of mt_spec_accept are checked against backend.select_token called
on the same logits rows with the seed of that row's token number, taking row b's answer. Every
output and in/out array sits between guard words that must come back unchanged."""
import numpy as np
import pytest

from spec_ref import accept, draft

pytestmark = pytest.mark.gpu

GUARD = -777


@pytest.fixture(scope="module")
def world():
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    import minitorch
    from minitorch import _hip
    _hip.lib()
    return dict(torch=torch, hip=_hip, backend=minitorch.TensorBackend(minitorch.HipKernelOps))


def guarded(torch, host, dtype=None):
    """A device copy of `host` as a contiguous view inside a larger buffer of guard words; returns
    (view, check), check() asserting the guard words are intact."""
    a = np.ascontiguousarray(host)
    pad = 8 if a.ndim == 1 else 2 * a.shape[-1]
    buf = torch.full((a.size + 2 * pad,), GUARD, dtype=dtype or torch.int32, device="cuda")
    view = buf[pad:pad + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a).to(view.dtype))

    def check():
        h = buf.cpu().numpy()
        assert (h[:pad] == GUARD).all() and (h[pad + a.size:] == GUARD).all(), "a guard word was overwritten"
    return view, check


def draft_rows(S):
    rng = np.random.default_rng(S)
    t = np.zeros((5, S), dtype=np.int32)
    t[0] = np.arange(S) + 100                 # all distinct: no match at any g
    t[1] = np.arange(S) % 2 + 7               # period 2
    t[2] = 4                                  # period 1
    t[3] = np.arange(S) % 9                   # period 9 > k
    t[4] = rng.integers(0, 3, S)              # many matches: the rightmost, the longest g
    return t


@pytest.mark.parametrize("S", [9, 48, 300, 1025])
def test_spec_draft_matches_the_rule(world, S):
    torch, hip = world["torch"], world["hip"]
    tokens_h = draft_rows(S)
    tokens = torch.from_numpy(tokens_h).cuda()
    helds = ([S] * 5, [1, 2, 2, 1, S + 50], [0, -3, S - 1, max(2, S // 2), S - 2])
    some_match = some_none = False
    for held_h in helds:
        held = torch.tensor(held_h, dtype=torch.int32, device="cuda")
        for k in (1, 4, 7):
            for ngram in (1, 3, 8):
                n = k + 1
                f32, c1 = guarded(torch, np.full((5, n), -1), torch.float32)
                i32, c2 = guarded(torch, np.full((5, n), -1))
                nd, c3 = guarded(torch, np.full(5, -1))
                hip.spec_draft(tokens, held, k, ngram, feed_f32=f32, feed_i32=i32, n_draft=nd)
                got_i, got_f, got_n = i32.cpu().numpy(), f32.cpu().numpy(), nd.cpu().numpy()
                for check in (c1, c2, c3):
                    check()
                for b in range(5):
                    feed, cnt = draft(tokens_h[b], held_h[b], k, ngram)
                    where = (S, held_h[b], k, ngram, b)
                    assert got_i[b].tolist() == feed and got_n[b] == cnt, where
                    assert got_f[b].tolist() == [float(t) for t in feed], where
                    some_match |= cnt == k
                    some_none |= cnt == 0
    assert some_match and some_none
    assert (tokens.cpu().numpy() == tokens_h).all(), "tokens is read only"
    # one output alone
    f32, i32, nd = hip.spec_draft(tokens, torch.full((5,), S, dtype=torch.int32, device="cuda"), 2, 3)
    assert (f32.cpu().numpy() == i32.cpu().numpy()).all() and i32.shape == (5, 3)


def test_spec_draft_strided_rows(world):
    """A row stride above S: what lies between the rows is not part of them."""
    torch, hip = world["torch"], world["hip"]
    S = 48
    tokens_h = draft_rows(S)
    wide = torch.full((5, S + 5), 1, dtype=torch.int32, device="cuda")
    wide[:, :S] = torch.from_numpy(tokens_h).cuda()
    held_h = [S, S, 3, S, S]
    _, i32, nd = hip.spec_draft(wide[:, :S], torch.tensor(held_h, dtype=torch.int32, device="cuda"), 4, 3)
    for b in range(5):
        feed, cnt = draft(tokens_h[b], held_h[b], 4, 3)
        assert i32[b].cpu().tolist() == feed and int(nd[b]) == cnt, b


@pytest.mark.parametrize("V,k,sampling", [(1, 3, False), (97, 3, False), (32768, 3, False), (1, 3, True),
                                          (97, 3, True), (32768, 3, True), (97, 7, False), (97, 1, True)])
def test_spec_accept_matches_select_token_and_the_rule(world, V, k, sampling):
    from minitorch.hip_kernel_ops import _wrap
    torch, backend = world["torch"], world["backend"]
    n = k + 1
    rng = np.random.default_rng(1000 * k + V)
    T, top_k, base = (0.8, 5, 4242) if sampling else (0.0, 0, 0)
    S, HS = 40, 32
    # rows 0..k: a = 0..k; then, all with every draft right: n_draft = 1 (matching padding slots), an
    # eos at accepted position min(1, k), limit - count = 1 and 2, done on entry, a NaN row, a tied
    # row, and n_draft = 0
    names = [f"a={a}" for a in range(n)] + ["pad", "eos", "limit1", "limit2", "done", "nan", "tie", "nodraft"]
    B = len(names)
    row = {name: i for i, name in enumerate(names)}
    logits_h = rng.standard_normal((B, n, V)).astype(np.float32)
    logits_h[row["nan"], 0, 5 % V] = np.nan
    logits_h[row["tie"], min(1, k)] = 0.25
    wide = torch.full((B, n, V + 3), 9e9, dtype=torch.float32, device="cuda")  # a row stride above V
    wide[:, :, :V] = torch.from_numpy(logits_h).cuda()
    logits = wide[:, :, :V]

    def rows_of(i):  # logits[:, i] as the minitorch tensor backend.select_token takes, in place
        return _wrap(wide.reshape(-1)[i * (V + 3):], (B, V), backend, (n * (V + 3), 1))
    count_h = np.array([1 + (3 * b) % 7 for b in range(B)], dtype=np.int32)  # rows at different token numbers
    held_h = count_h + 5 + np.arange(B, dtype=np.int32) % 4
    limit_h = np.full(B, 30, dtype=np.int32)
    limit_h[row["limit1"]] = count_h[row["limit1"]] + 1
    limit_h[row["limit2"]] = count_h[row["limit2"]] + 2
    done_h = np.zeros(B, dtype=np.int32)
    done_h[row["done"]] = 1
    # c_i by select_token: logits[:, i] with the seed of row b's token number count[b] + i, row b's answer
    c = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        for i in range(n):
            c[b, i] = int(backend.select_token(rows_of(i), T, top_k, base + int(count_h[b]) + i)[1][b])
    if not sampling and V > 5:
        assert c[row["nan"], 0] == 5 and c[row["tie"], min(1, k)] == 0
    feed_h = np.zeros((B, n), dtype=np.int32)
    feed_h[:, 0] = 3
    feed_h[:, 1:] = c[:, :k]
    for a in range(k):
        feed_h[a, 1 + a] = c[a, a] + 1  # the first wrong draft of row a (an id the row did not choose)
    ndraft_h = np.full(B, k, dtype=np.int32)
    ndraft_h[row["pad"]] = min(1, k - 1)
    ndraft_h[row["nodraft"]] = 0
    eos = int(c[row["eos"], min(1, k)])
    tokens_h = rng.integers(0, 50, (B, S)).astype(np.int32)
    history_h = rng.integers(0, 50, (B, HS)).astype(np.int32)
    cache_h, drafted_h, accepted_h, steps_h = held_h - 1, count_h * 2, count_h + 1, count_h % 3

    dev = {name: guarded(torch, h) for name, h in dict(
        feed=feed_h, ndraft=ndraft_h, limit=limit_h, count=count_h, held=held_h, cache=cache_h, done=done_h,
        drafted=drafted_h, accepted=accepted_h, steps=steps_h, tokens=tokens_h, history=history_h,
        scratch=np.full((B, n), -5, dtype=np.int32)).items()}
    d = {name: v[0] for name, v in dev.items()}
    seed_dev = torch.tensor([base], dtype=torch.int64, device="cuda") if sampling else None
    kw = dict(scratch=d["scratch"], cache_len=d["cache"], drafted=d["drafted"], accepted=d["accepted"],
              steps=d["steps"], eos_id=eos)
    if sampling:  # the device seed wins over the host one
        kw.update(temperature=T, top_k=top_k, seed=base + 99, seed_dev=seed_dev)
    backend.spec_accept(logits, d["feed"], d["ndraft"], d["limit"], d["count"], d["held"], d["done"], d["tokens"],
                        d["history"], **kw)
    for _, check in dev.values():
        check()
    got = {name: v.cpu().numpy() for name, v in d.items()}
    want = dict(count=count_h.copy(), held=held_h.copy(), cache=cache_h.copy(), done=done_h.copy(),
                drafted=drafted_h.copy(), accepted=accepted_h.copy(), steps=steps_h.copy(), tokens=tokens_h.copy(),
                history=history_h.copy(), feed=feed_h, ndraft=ndraft_h, limit=limit_h)
    seen_a = set()
    for b in range(B):
        if done_h[b]:
            assert (got["scratch"][b] == -5).all(), "a row done on entry is not chosen for"
            continue
        assert got["scratch"][b].tolist() == c[b].tolist(), (names[b], "c_i is select_token's id")
        r = accept(c[b].tolist(), feed_h[b].tolist(), ndraft_h[b], int(count_h[b]), int(held_h[b]), int(limit_h[b]), eos)
        w = len(r["written"])
        want["history"][b, count_h[b]:count_h[b] + w] = r["written"]
        want["tokens"][b, held_h[b]:held_h[b] + w] = r["written"]
        want["count"][b], want["held"][b] = r["count"], r["held"]
        want["cache"][b] += w
        want["done"][b] = int(r["done"])
        want["drafted"][b] += r["drafted"]
        want["accepted"][b] += r["accepted"]
        want["steps"][b] += 1
        seen_a.add(r["a"])
        assert want["cache"][b] == want["held"][b] - 1
    for name, w in want.items():
        assert (got[name] == w).all(), (name, got[name].tolist(), w.tolist())
    # the cases are what they claim to be (V = 1 has one id: every draft is "right", an eos everywhere)
    if V > 5:
        assert seen_a >= set(range(n)), seen_a
        grew = lambda name: int(want["count"][row[name]] - count_h[row[name]])  # noqa: E731
        clear = lambda name, m: eos not in c[row[name], :m].tolist()  # noqa: E731
        assert grew("pad") == ndraft_h[row["pad"]] + 1 or not clear("pad", ndraft_h[row["pad"]] + 1)
        assert want["done"][row["eos"]] == 1 and grew("eos") <= min(1, k) + 1
        assert grew("limit2") == min(2, n) or not clear("limit2", 2)
    assert want["count"][row["limit1"]] - count_h[row["limit1"]] == 1 and want["done"][row["limit1"]] == 1
