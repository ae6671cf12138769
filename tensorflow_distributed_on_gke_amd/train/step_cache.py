"""The captured training steps of a TrainStep: an LRU cache with one current
entry. Holds no torch object of its own and imports none.

A key is what a captured micro-batch bakes in, as TrainStep._cache_key builds
it: (source shape, target shape, position in the update, loss divisor, loss
mode). The current entry is the one a replay runs; nothing but this class
writes it.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Dict, Iterable, List, NamedTuple, Optional, Tuple


class Captured(NamedTuple):
    """One captured micro-batch: a single HIP graph or a segmented one (the
    other is None) and the static (src, tgt) input buffers it reads."""
    graph: Any
    segments: Any
    static: Any


_NONE = Captured(None, None, None)


class StepCache:
    def __init__(self, capacity: int = 64, bucketed: bool = False):
        # newest last
        self.entries: "OrderedDict[tuple, Captured]" = OrderedDict()
        self.current: Optional[tuple] = None
        self.stats: Dict[str, int] = {"captures": 0, "replays": 0, "evictions": 0}
        # a miss captures on the spot (False: a miss is an error)
        self.bucketed = bucketed
        # entries kept when a miss makes room (at least one)
        self.capacity = capacity

    def __len__(self) -> int:
        return len(self.entries)

    @property
    def entry(self) -> Captured:
        """The current entry (all fields None when there is none)."""
        return self.entries[self.current] if self.current is not None else _NONE

    def get(self, key: tuple) -> Optional[Captured]:
        """A hit becomes the most recently used and the current entry."""
        ent = self.entries.get(key)
        if ent is not None:
            self.entries.move_to_end(key)
            self.current = key
        return ent

    def put(self, key: tuple, captured: Captured) -> None:
        """A just-captured micro-batch becomes the current entry."""
        self.entries[key] = Captured(*captured)
        self.entries.move_to_end(key)
        self.current = key
        self.stats["captures"] += 1

    def make_room(self) -> None:
        """Evict least recently used entries until one more fits."""
        while len(self.entries) >= max(1, self.capacity):
            key, _ = self.entries.popitem(last=False)
            if key == self.current:
                self.current = None
            self.stats["evictions"] += 1

    def install(self, entries: Optional[Iterable]) -> None:
        """Replace the contents by `entries` (a mapping or (key, captured)
        pairs; None: nothing captured). The newest entry becomes current."""
        self.entries = OrderedDict((k, Captured(*c)) for k, c in dict(entries or ()).items())
        self.current = next(reversed(self.entries)) if self.entries else None

    def clear_current(self) -> None:
        self.current = None

    def shapes(self) -> List[Tuple[tuple, tuple]]:
        """The distinct (source, target) shapes held, sorted."""
        return sorted({(k[0], k[1]) for k in self.entries})
