"""PageAllocator (minitorch/kv_cache.py): the free list and the reference counts behind a
PagedKVCache's block table. Pure host code: no device, nothing launched."""
import pytest

from minitorch import PageAllocator, PoolExhausted


def _state(a):
    return a.n_free, [a.refcount(p) for p in range(a.n_pages)]


def test_alloc_and_release_return_the_pool_to_full():
    a = PageAllocator(8)
    assert _state(a) == (8, [0] * 8)
    first = a.alloc(3)
    second = a.alloc(5)
    assert sorted(first + second) == list(range(8))  # every page once
    assert _state(a) == (0, [1] * 8)
    for p in second + first:
        a.release(p)
    assert _state(a) == (8, [0] * 8)
    # the pool is whole again: it can be taken in full once more, every page once
    assert sorted(a.alloc(8)) == list(range(8))
    assert a.alloc(0) == []


def test_reference_counts_under_retain_and_release():
    a = PageAllocator(4)
    p, q = a.alloc(2)
    a.retain(p)
    a.retain(p)
    assert (a.refcount(p), a.refcount(q), a.n_free) == (3, 1, 2)
    a.release(p)
    assert (a.refcount(p), a.n_free) == (2, 2)  # still held: not back on the free list
    a.release(q)
    assert (a.refcount(q), a.n_free) == (0, 3)
    a.release(p)
    assert (a.refcount(p), a.n_free) == (1, 3)
    a.release(p)
    assert (a.refcount(p), a.n_free) == (0, 4)
    # a freed page comes back with one reference
    got = a.alloc(4)
    assert sorted(got) == [0, 1, 2, 3] and all(a.refcount(x) == 1 for x in got)


def test_exhaustion_raises_and_changes_nothing():
    a = PageAllocator(5)
    held = a.alloc(3)
    a.retain(held[0])
    before = _state(a)
    free_before = list(a._free)
    with pytest.raises(PoolExhausted, match="3 pages wanted, 2 of 5 free"):
        a.alloc(3)
    assert _state(a) == before and a._free == free_before
    # what is free can still be taken, and then nothing more
    assert len(a.alloc(2)) == 2
    with pytest.raises(PoolExhausted):
        a.alloc(1)
    assert a.n_free == 0


def test_releasing_a_page_twice_raises():
    a = PageAllocator(3)
    (p,) = a.alloc(1)
    a.release(p)
    before = _state(a)
    with pytest.raises(ValueError, match="already free"):
        a.release(p)
    assert _state(a) == before  # and the page is on the free list once
    assert sorted(a.alloc(3)) == [0, 1, 2]


def test_misuse_raises():
    a = PageAllocator(2)
    with pytest.raises(ValueError, match="is free"):
        a.retain(0)
    for bad in (-1, 2, 0.5):
        with pytest.raises(ValueError, match="not a page"):
            a.release(bad)
    with pytest.raises(ValueError):
        a.alloc(-1)
    for n in (0, -4, 1.5):
        with pytest.raises(ValueError, match="n_pages"):
            PageAllocator(n)
