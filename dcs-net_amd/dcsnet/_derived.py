"""One guarded cache for device tensors derived from other tensors: packed weights, inference-time constants, windows.

    PACKS = Derived(capacity=512)
    wp, bias = PACKS.get(owner, tag, sources, make, extra)

An entry lives and dies with its `owner` (a module or a tensor) and is valid while its stamp holds:

    (state generation, extra, per source (id, _version, data_ptr))        and every source is still the same object.

The entry is dropped the moment its owner or one of its sources dies (weakref callbacks), so the sources of a live entry are
alive and an equal id() in the stamp means the same object; the owner's weakref is checked on every hit all the same.

`_version` sees in-place updates, `data_ptr` sees `p.data = other` (Module.to() / .float() swap .data and leave the version
alone), the state generation sees kernels that write parameters or running statistics behind torch's back, `extra` is
whatever else the value depends on (the conv precision of a packed panel).  A stale entry is replaced by its next lookup;
beyond `capacity` the least recently used entry goes, one at a time.  While the current stream is being captured nothing is
inserted: a value made there lives in the graph's pool.

A captured graph holds addresses, not references, and any entry may be evicted.  Whoever captures runs one warm pass inside
`with collect() as kept:` and keeps the list: a strong reference to every value any instance served or made meanwhile.
"""
import contextlib
import weakref
from collections import OrderedDict

import torch

_generation = 0
_collecting = None
_instances = weakref.WeakSet()


def bump_generation():
    """Parameters or module state were rewritten behind torch's version counters: every state-tracking entry is stale."""
    global _generation
    _generation += 1


def generation():
    return _generation


def capturing():
    """Is the current stream being captured into a graph?  (The one place that asks; CPU tests substitute it.)"""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


@contextlib.contextmanager
def collect():
    """-> list that receives a strong reference to every value served or made, by any instance, inside the block."""
    global _collecting
    outer, kept = _collecting, []
    _collecting = kept
    try:
        yield kept
    finally:
        _collecting = outer
        if outer is not None:
            outer.extend(kept)


def clear_all():
    """Drop every entry of every instance (tests; memory back after a precision switch).  Never needed for validity."""
    for inst in _instances:
        inst._entries.clear()


class Derived:
    """capacity: entries kept (least recently used evicted), or None for kinds whose owners are few and long-lived modules.
    tracks_state=False: the sources are tensors no kernel writes (analysis windows), the state generation stays out of the stamp."""

    def __init__(self, capacity=None, tracks_state=True):
        self.capacity, self.tracks_state = capacity, tracks_state
        self._entries = OrderedDict()          # (id(owner), tag) -> (stamp, (owner ref, source refs...), value), oldest use first
        _instances.add(self)

    def __len__(self):
        return len(self._entries)

    def _stamp(self, sources, extra):
        return (_generation if self.tracks_state else 0, extra,
                tuple([None if t is None else (id(t), t._version, t.data_ptr()) for t in sources]))

    def get(self, owner, tag, sources, make, extra=()):
        """The valid value (a hit: one dict get, one tuple compare, the owner's weakref), or make() stored and returned."""
        key = (id(owner), tag)
        ent = self._entries.get(key)
        if ent is None or ent[0] != self._stamp(sources, extra) or ent[1][0]() is not owner:
            return None if make is None else self.put(owner, tag, sources, make(), extra)
        if self.capacity is not None:
            self._entries.move_to_end(key)
        if _collecting is not None:
            _collecting.append(ent[2])
        return ent[2]

    def peek(self, owner, tag, sources, extra=()):
        """The valid value, or None; never makes one."""
        return self.get(owner, tag, sources, None, extra)

    def put(self, owner, tag, sources, val, extra=()):
        """Store `val` (just made by the caller) unless the stream is being captured; -> val."""
        if _collecting is not None:
            _collecting.append(val)
        if capturing():
            return val
        key, entries = (id(owner), tag), self._entries

        def drop(ref):                         # the owner or a source died: its id() may be handed out again
            ent = entries.get(key)
            if ent is not None and any(r is ref for r in ent[1]):
                del entries[key]
        refs = tuple(weakref.ref(t, drop) for t in (owner, *sources) if t is not None)
        entries[key] = (self._stamp(sources, extra), refs, val)
        entries.move_to_end(key)
        while self.capacity is not None and len(entries) > self.capacity:
            entries.popitem(last=False)
        return val
