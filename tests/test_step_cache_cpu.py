"""StepCache (train/step_cache.py): the LRU cache of captured training steps
with one current entry, driven with stub entries -- no torch device."""
from tensorflow_distributed_on_gke_amd.train.step_cache import Captured, StepCache


def key(s=4, t=5, pos="only", workers=1.0, global_mean=False):
    return ((2, s), (2, t), pos, workers, global_mean)


def ent(name):
    return Captured("graph-" + name, None, ("src-" + name, "tgt-" + name))


def test_put_counts_a_capture_and_captured_unpacks_as_a_3_tuple():
    c = StepCache()
    assert not c.entries and c.current is None and c.entry == (None, None, None)
    c.put(key(), ent("a"))
    assert c.stats == {"captures": 1, "replays": 0, "evictions": 0}
    assert c.current == key() and len(c) == 1
    graph, segments, static = c.entry
    assert (graph, segments, static) == ("graph-a", None, ("src-a", "tgt-a"))
    for k, (_, segs, _) in c.entries.items():
        assert k == key() and segs is None
    c.put(key(6), ("g", "s", "st"))  # a plain 3-tuple is taken as an entry
    assert c.entry.segments == "s" and c.stats["captures"] == 2


def test_hit_makes_the_entry_current_and_most_recent():
    c = StepCache()
    for s in (4, 6, 8):
        c.put(key(s), ent(str(s)))
    assert c.current == key(8) and list(c.entries) == [key(4), key(6), key(8)]
    assert c.get(key(4)) == ent("4")
    assert c.current == key(4) and c.entry == ent("4")
    assert list(c.entries) == [key(6), key(8), key(4)]
    assert c.get(key(10)) is None  # a miss changes nothing
    assert c.current == key(4) and list(c.entries) == [key(6), key(8), key(4)]
    assert c.stats["captures"] == 3 and c.stats["evictions"] == 0
    c.clear_current()
    assert c.current is None and c.entry.graph is None and len(c) == 3


def miss(c, k, e):
    """What a bucketed miss does: make room, capture, put."""
    assert c.get(k) is None
    c.make_room()
    c.put(k, e)


def test_capacity_2_evicts_the_least_recently_used():
    c = StepCache(capacity=2, bucketed=True)
    a, b, d, e = key(4), key(6), key(8), key(10)
    miss(c, a, ent("a"))
    miss(c, b, ent("b"))
    assert c.stats["evictions"] == 0
    miss(c, d, ent("d"))  # a is the least recently used
    assert list(c.entries) == [b, d] and c.stats["evictions"] == 1
    c = StepCache(capacity=2, bucketed=True)
    miss(c, a, ent("a"))
    miss(c, b, ent("b"))
    assert c.get(a) is not None  # touched: now b is
    miss(c, d, ent("d"))
    assert list(c.entries) == [a, d] and c.current == d and c.stats["evictions"] == 1
    miss(c, e, ent("e"))
    assert list(c.entries) == [d, e] and c.stats["evictions"] == 2
    assert c.stats["captures"] == 4
    c.capacity = 1  # shrunk: the next miss evicts down to one free slot
    miss(c, a, ent("a"))
    assert list(c.entries) == [a] and c.stats["evictions"] == 4


def test_capacity_0_behaves_as_1():
    for cap in (0, 1):
        c = StepCache(capacity=cap, bucketed=True)
        c.make_room()  # nothing to evict
        c.put(key(4), ent("a"))
        miss(c, key(6), ent("b"))
        assert list(c.entries) == [key(6)] and c.current == key(6)
        assert c.stats == {"captures": 2, "replays": 0, "evictions": 1}
        assert c.current is not None and c.entry == ent("b")


def test_evicting_the_current_entry_leaves_none_current():
    c = StepCache(capacity=1, bucketed=True)
    c.put(key(4), ent("a"))
    c.make_room()
    assert not c.entries and c.current is None and c.entry.static is None


def test_pos_workers_and_global_mean_make_distinct_entries():
    c = StepCache()
    keys = [key(), key(pos="first"), key(pos="last"), key(workers=2.0), key(global_mean=True)]
    for i, k in enumerate(keys):
        c.put(k, ent(str(i)))
    assert len(c) == len(keys) == len(set(keys))
    for i, k in enumerate(keys):
        assert c.get(k) == ent(str(i)) and c.current == k
    assert c.shapes() == [((2, 4), (2, 5))]  # one batch shape all the same
    c.put(key(6, 3), ent("x"))
    assert c.shapes() == [((2, 4), (2, 5)), ((2, 6), (2, 3))]
    assert {k[2] for k in c.entries} == {"only", "first", "last"}


def test_install_makes_the_newest_current_and_none_leaves_nothing():
    c = StepCache()
    c.put(key(4), ent("a"))
    arm = {key(6, pos="first"): ent("f"), key(6, pos="last"): ent("l")}
    c.install(arm)
    assert list(c.entries) == list(arm) and c.current == key(6, pos="last")
    assert c.entry == ent("l") and c.current[2] == "last"
    assert c.entries is not arm
    c.install(None)
    assert not c.entries and c.current is None and c.entry == (None, None, None)
    assert arm and c.stats["captures"] == 1  # the arm is untouched; install counts nothing
    c.install(list(arm.items()))
    assert c.current == key(6, pos="last") and len(c) == 2
