"""CPU: the one guarded cache of derived tensors (dcsnet/_derived.py) — validity stamp, owner lifetime, least-recently-used
eviction, the capture rule and collect() — on CPU tensors, without the HIP library."""
import gc
import weakref

import pytest
import torch

from dcsnet import _derived
from dcsnet._derived import Derived


class _Maker:
    """make() with a call counter; every value is a fresh tensor."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return torch.full((2,), float(self.calls))


def test_a_hit_returns_the_same_object():
    c, mk, w = Derived(4), _Maker(), torch.randn(3, 3)
    a = c.get(w, 'tag', (w, None), mk)
    assert c.get(w, 'tag', (w, None), mk) is a and c.peek(w, 'tag', (w, None)) is a
    assert mk.calls == 1 and len(c) == 1
    assert c.peek(w, 'other', (w, None)) is None and c.get(w, 'other', (w, None), mk) is not a and mk.calls == 2


def test_an_in_place_update_misses():
    c, mk, w = Derived(4), _Maker(), torch.randn(3, 3)
    a = c.get(w, 0, (w,), mk)
    w.mul_(1.25)
    assert c.peek(w, 0, (w,)) is None
    assert c.get(w, 0, (w,), mk) is not a and mk.calls == 2 and len(c) == 1


def test_a_data_swap_misses():
    """`p.data = other` (what Module.to() and Module.float() do) leaves `_version` where it was and gives a new data_ptr.
    The former key of functional.packed_weight, (id, _version) per tensor, could not see this and served the old pack."""
    c, mk, p = Derived(4), _Maker(), torch.nn.Parameter(torch.randn(3, 3))
    a = c.get(p, 0, (p,), mk)
    version, identity = p._version, id(p)
    p.data = torch.randn(3, 3)
    assert p._version == version and id(p) == identity          # nothing the old key looked at has moved
    assert c.peek(p, 0, (p,)) is None
    assert c.get(p, 0, (p,), mk) is not a and mk.calls == 2


def test_a_generation_bump_misses_and_the_public_names_forward():
    from dcsnet import functional as F
    c, still, mk, w = Derived(4), Derived(4, tracks_state=False), _Maker(), torch.randn(3)
    a, s = c.get(w, 0, (w,), mk), still.get(w, 0, (w,), mk)
    for bump in (_derived.bump_generation, F.bump_param_generation, F.note_state_update):
        g = F.state_generation()
        bump()
        assert F.state_generation() == _derived.generation() == g + 1
        assert c.peek(w, 0, (w,)) is None
        b = c.get(w, 0, (w,), mk)
        assert b is not a and c.get(w, 0, (w,), mk) is b
        a = b
    assert still.get(w, 0, (w,), mk) is s                        # a kind whose sources no kernel writes


def test_a_changed_extra_misses():
    c, mk, w = Derived(4), _Maker(), torch.randn(3)
    a = c.get(w, 0, (w,), mk, 'bf16x6')
    assert c.peek(w, 0, (w,), 'bf16') is None and c.peek(w, 0, (w,), 'bf16x6') is a
    b = c.get(w, 0, (w,), mk, 'bf16')
    assert b is not a and c.peek(w, 0, (w,), 'bf16x6') is None and len(c) == 1
    assert c.get(w, 0, (w,), mk, 'bf16x6') is not a and mk.calls == 3


def test_a_none_source_becoming_a_tensor_and_back_misses():
    c, mk, w, b = Derived(4), _Maker(), torch.randn(3), torch.randn(3)
    v0 = c.get(w, 0, (w, None), mk)
    v1 = c.get(w, 0, (w, b), mk)
    assert v1 is not v0 and c.get(w, 0, (w, b), mk) is v1
    v2 = c.get(w, 0, (w, None), mk)
    assert v2 is not v1 and v2 is not v0 and mk.calls == 3


def test_an_entry_dies_with_its_owner():
    c, mk = Derived(4), _Maker()
    owner, src = torch.nn.Linear(2, 2), torch.randn(3)
    c.get(owner, 'a', (src,), mk)
    c.get(owner, 'b', (src,), mk)
    assert len(c) == 2
    del owner
    gc.collect()
    assert len(c) == 0


def test_an_entry_dies_with_any_of_its_sources():
    """The sources of a live entry are alive, so an equal id() in its stamp means the same object: a tensor that was handed
    a dead source's id (and happens to share its version and address) is never served the dead one's value."""
    c, mk = Derived(4), _Maker()
    owner, a, b = torch.nn.Linear(2, 2), torch.randn(3), torch.randn(3)
    c.get(owner, 't', (a, None, b), mk)
    assert len(c) == 1
    del b
    gc.collect()
    assert len(c) == 0 and c.peek(owner, 't', (a, None, torch.randn(3))) is None


def test_a_recycled_id_is_not_served_a_dead_owners_value():
    c, mk, src = Derived(), _Maker(), torch.randn(3)
    # by hand: an entry under a live object's id whose owner reference is dead (what a missed callback would leave)
    dead = torch.nn.Identity()
    ref = weakref.ref(dead)
    del dead
    gc.collect()
    assert ref() is None
    owner = torch.nn.Identity()
    stale = torch.zeros(1)
    c._entries[(id(owner), 0)] = (c._stamp((src,), ()), (ref, weakref.ref(src)), stale)
    assert c.peek(owner, 0, (src,)) is None
    mine = c.get(owner, 0, (src,), mk)
    assert mine is not stale and c.get(owner, 0, (src,), mk) is mine and mk.calls == 1
    # in the wild: allocate until an id repeats
    seen = {}
    for i in range(4000):
        o = torch.nn.Identity()
        if id(o) in seen:
            assert c.peek(o, 'w', (src,)) is None
            assert c.get(o, 'w', (src,), mk) is not seen[id(o)]
            return
        seen[id(o)] = c.get(o, 'w', (src,), mk)
        del o
    pytest.skip('no id() was handed out twice in 4000 allocations; the hand-made stale entry above covers the check')


def test_eviction_is_least_recently_used_one_at_a_time():
    c, mk, w = Derived(4), _Maker(), torch.randn(3)
    vals = {}
    for tag in range(6):
        vals[tag] = c.get(w, tag, (w,), mk)
        assert len(c) <= 4
        if tag == 3:
            assert c.get(w, 0, (w,), mk) is vals[0]              # touched: now the most recently used
    assert len(c) == 4
    assert [c.peek(w, t, (w,)) is vals[t] for t in range(6)] == [True, False, False, True, True, True]


def test_nothing_is_stored_while_capturing(monkeypatch):
    c, mk, w = Derived(4), _Maker(), torch.randn(3)
    monkeypatch.setattr(_derived, 'capturing', lambda: True)
    a = c.get(w, 0, (w,), mk)
    assert torch.equal(a, torch.full((2,), 1.0)) and len(c) == 0 and c.peek(w, 0, (w,)) is None
    b = c.get(w, 0, (w,), mk)
    assert b is not a and mk.calls == 2 and len(c) == 0
    monkeypatch.setattr(_derived, 'capturing', lambda: False)
    d = c.get(w, 0, (w,), mk)
    monkeypatch.setattr(_derived, 'capturing', lambda: True)
    assert c.get(w, 0, (w,), mk) is d and mk.calls == 3         # what was there before the capture is served


def test_collect_holds_what_was_served_and_made_inside_the_block():
    c1, c2, mk, w = Derived(2), Derived(), _Maker(), torch.randn(3)
    before = c1.get(w, 'before', (w,), mk)
    served = c2.get(w, 'served', (w,), mk)
    with _derived.collect() as kept:
        made = c1.get(w, 'made', (w,), mk)
        assert c2.get(w, 'served', (w,), mk) is served
        assert c2.peek(w, 'served', (w,)) is served
        assert c2.peek(w, 'absent', (w,)) is None
    after = c1.get(w, 'after', (w,), mk)
    assert [id(v) for v in kept] == [id(made), id(served), id(served)]
    assert all(v is not before and v is not after for v in kept)
    for tag in range(3):                                         # everything of c1 evicted, everything dropped
        c1.get(w, tag, (w,), mk)
    _derived.clear_all()
    assert len(c1) == len(c2) == 0
    assert kept[0] is made and kept[1] is served and torch.equal(made, torch.full((2,), 3.0))


def test_a_parameter_as_owner_and_source():
    """A WeakKeyDictionary keyed by a tensor fails on a hit: weakref equality calls Tensor.__eq__ and bool() of a 3x3 result
    raises.  The cache keys by id() and compares references with `is`."""
    c, mk = Derived(4), _Maker()
    p, q = torch.nn.Parameter(torch.randn(3, 3)), torch.nn.Parameter(torch.randn(3, 3))
    a, b = c.get(p, 0, (p, q), mk), c.get(q, 0, (q, p), mk)
    assert c.get(p, 0, (p, q), mk) is a and c.get(q, 0, (q, p), mk) is b and a is not b
    del p, q
    gc.collect()
    assert len(c) == 0


def test_window_and_envelope_lookups(monkeypatch):
    from dcsnet import network_functions as nf, ops

    class Cfg:
        window = torch.hann_window(512)
    meta = torch.device('meta')
    _derived.clear_all()
    w = nf._window_on(Cfg, meta)
    assert w.device == meta and nf._window_on(Cfg, meta) is w
    assert nf._window_on(Cfg, Cfg.window.device) is Cfg.window
    calls = []

    def envelope(window, T, hop):
        calls.append((T, hop))
        return torch.zeros(hop * (T - 1))
    monkeypatch.setattr(ops, 'istft_envelope', envelope)
    win = torch.hann_window(512)
    e = nf._inv_envelope(win, 16, 32)
    assert nf._inv_envelope(win, 16, 32) is e and calls == [(16, 32)]
    F_gen = _derived.generation()
    _derived.bump_generation()                                   # a train step: windows are no module state
    assert nf._inv_envelope(win, 16, 32) is e and _derived.generation() == F_gen + 1
    win.mul_(0.5)
    assert nf._inv_envelope(win, 16, 32) is not e and calls == [(16, 32), (16, 32)]
    Cfg.window.mul_(0.5)
    assert nf._window_on(Cfg, meta) is not w
    for t in range(70):
        nf._inv_envelope(win, 24 + 8 * t, 32)
    assert len(calls) == 72 and len(nf._ENVELOPES) == 64
