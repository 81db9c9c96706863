"""The launch-plan container without a GPU: `_Plan(lib)` takes its library as an argument and `rt.check(0)` never touches the real one,
so a stub that hands out integer handles shows which events and graphs a plan creates and that `close()` gives every one of them back
once, graphs first.  And PlanKey: a named tuple that is still the positional tuple the plan registry was keyed by."""
import ctypes as C

import pytest

from video_gcp_amd.plan_ops import _Plan, PlanKey


class StubLib:
    """every entry point records (name, args) and returns 0; the creating ones write a fresh handle through their out-pointer"""
    CREATE = ("gcpx_event_create_sync", "gcpx_event_create", "gcpx_graph_end")

    def __init__(self):
        self.calls, self.handed = [], {"event": [], "graph": []}

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name in StubLib.CREATE:
                h = 1000 + len(self.handed["event"]) + len(self.handed["graph"])
                self.handed["graph" if name == "gcpx_graph_end" else "event"].append(h)
                args[-1]._obj.value = h
            return 0
        return fn

    def destroyed(self, kind):
        return [a[0].value for n, a in self.calls if n == f"gcpx_{kind}_destroy"]


def _plan():
    """fork, three launches on lane 0, one on lane 1, wait / record / await / join and a mark; compacted with min_len = 3"""
    lib = StubLib()
    plan = _Plan(lib)
    plan.fork([1, 2])
    for name in "abc":
        plan.add(name, getattr(lib, "launch_" + name), 7)
    plan.lane = 1
    plan.add("d", lib.launch_d, 7)
    plan.lane = 0
    plan.wait(0, 1)
    ev = plan.record(2)
    plan.await_event(0, ev)
    plan.join([1, 2])
    plan.mark("tag", 0)
    streams = [C.c_void_p(11), C.c_void_p(12), C.c_void_p(13)]
    ops = plan.compact(streams, 3)
    return lib, plan, streams, ops


def test_a_plan_creates_five_events_and_one_segment_graph():
    lib, plan, streams, ops = _plan()
    assert ops is plan.segments
    assert [op[0] for op in ops] == ["@fork", "@graph", "d", "@wait", "@record", "@await", "@join", "@mark"]
    assert len(lib.handed["event"]) == 5 and len(lib.handed["graph"]) == 1
    assert len(set(lib.handed["event"] + lib.handed["graph"])) == 6
    plan.run(streams, ops=ops)                                   # replays: nothing is created or destroyed by running
    assert len(lib.handed["event"]) == 5 and len(lib.handed["graph"]) == 1
    assert lib.destroyed("event") == [] and lib.destroyed("graph") == []


def test_close_releases_every_handle_once_graphs_first_and_the_plan_runs_no_more():
    lib, plan, streams, ops = _plan()
    plan.close()
    assert sorted(lib.destroyed("event")) == sorted(lib.handed["event"])
    assert sorted(lib.destroyed("graph")) == sorted(lib.handed["graph"])
    names = [n for n, _ in lib.calls if n.endswith("_destroy")]
    assert names == ["gcpx_graph_destroy"] * 1 + ["gcpx_event_destroy"] * 5
    assert plan.closed and plan.graph is None and plan.split is None and plan.segments is None
    n = len(lib.calls)
    plan.close()
    assert len(lib.calls) == n                                   # a second close() calls nothing
    with pytest.raises(RuntimeError):
        plan.run(streams)
    with pytest.raises(RuntimeError):
        plan.run(streams, ops=ops)
    assert len(lib.calls) == n


def test_close_releases_the_forward_graph_and_the_split_pair_too():
    lib, plan, streams, ops = _plan()
    plan.graph, plan.split = C.c_void_p(2001), (C.c_void_p(2002), C.c_void_p(2003))
    plan.close()
    assert sorted(lib.destroyed("graph")) == sorted(lib.handed["graph"] + [2001, 2002, 2003])
    assert sorted(lib.destroyed("event")) == sorted(lib.handed["event"])
    names = [n for n, _ in lib.calls if n.endswith("_destroy")]
    assert names == ["gcpx_graph_destroy"] * 4 + ["gcpx_event_destroy"] * 5


def test_a_failed_destroy_is_reported_through_check(monkeypatch):
    from video_gcp_amd import runtime as rt
    lib, plan, streams, ops = _plan()
    lib.gcpx_graph_destroy = lambda g: 3
    seen = []
    monkeypatch.setattr(rt, "check", lambda status, what="": seen.append((status, what)) if status else None)
    plan.close()
    assert seen == [(3, "graph_destroy")]


def test_plan_key_built_by_keyword_is_the_old_positional_tuple():
    shapes = (("I_0", (3, 3, 64, 64)), ("end_ind", (3,)))
    old = (3, True, False, False, "train", True, False, True, True, False, shapes)
    key = PlanKey(B=3, has_traj=True, has_z=False, sample_prior=False, phase="train", training=True, materialize_distr=False,
                  with_loss=True, decode=True, pred_len=False, shapes=shapes)
    assert PlanKey._fields == ("B", "has_traj", "has_z", "sample_prior", "phase", "training", "materialize_distr", "with_loss", "decode",
                               "pred_len", "shapes")
    assert key == old and hash(key) == hash(old) and {old: 1}[key] == 1 and {key: 1}[old] == 1
    assert (key.B, key.phase, key.with_loss, key.decode, key.pred_len, key.shapes) == (3, "train", True, True, False, shapes)
    assert key != old[:7] + (False,) + old[8:]
