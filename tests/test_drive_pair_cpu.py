"""RCNN.drive_pair: two engines' request generators advanced together.  Fake engines and a fake grouped launch that log every call; the expected
logs are written out by hand.  No GPU."""
import pytest
import torch

from aldi_amd import engine as E


class FakeEngine:
    def __init__(self, tag, log):
        self.tag, self.log = tag, log

    def _conv_call(self, x, name, **kw):
        self.log.append((self.tag, "call", name))
        return x, "w:" + name, kw

    def _serve(self, req):
        if isinstance(req, list):
            self.log.append((self.tag, "serve", [r[1] for r in req]))
            return ["y:" + r[0] for r in req]
        self.log.append((self.tag, "serve", req[1]))
        return "y:" + req[0]


def _gen(tag, reqs, log, ret):
    got = []
    for r in reqs:
        y = yield r
        log.append((tag, "got", y))
        got.append(y)
    return ret, got


def R(name, **kw):
    return ("x" + name, name, kw)


@pytest.fixture
def log(monkeypatch):
    out = []

    def group(calls):
        out.append(("group", [w for _, w, _ in calls]))
        return ["y:" + x for x, _, _ in calls]
    monkeypatch.setattr(E.ops, "conv2d_group", group)
    return out


def _run(log, reqs_a, reqs_b, streams=None):
    a, b = FakeEngine("A", log), FakeEngine("B", log)
    return E.RCNN.drive_pair(a, _gen("A", reqs_a, log, "ra"), b, _gen("B", reqs_b, log, "rb"), streams=streams)


def test_three_and_one_requests_group_once_then_a_alone(log):
    res = _run(log, [R("a1"), R("a2"), R("a3")], [R("b1")])
    assert log == [("A", "call", "a1"), ("B", "call", "b1"), ("group", ["w:a1", "w:b1"]), ("A", "got", "y:xa1"), ("B", "got", "y:xb1"),
                   ("A", "serve", "a2"), ("A", "got", "y:xa2"),
                   ("A", "serve", "a3"), ("A", "got", "y:xa3")]
    assert res == (("ra", ["y:xa1", "y:xa2", "y:xa3"]), ("rb", ["y:xb1"]))


def test_one_and_two_requests_group_once_then_b_alone(log):
    res = _run(log, [R("a1")], [R("b1"), R("b2")])
    assert log == [("A", "call", "a1"), ("B", "call", "b1"), ("group", ["w:a1", "w:b1"]), ("A", "got", "y:xa1"), ("B", "got", "y:xb1"),
                   ("B", "serve", "b2"), ("B", "got", "y:xb2")]
    assert res == (("ra", ["y:xa1"]), ("rb", ["y:xb1", "y:xb2"]))


def test_list_request_beside_a_single_one_slices_the_results(log):
    res = _run(log, [[R("a1"), R("a2")], R("a3")], [R("b1"), [R("b2"), R("b3")]])
    assert log == [("A", "call", "a1"), ("A", "call", "a2"), ("B", "call", "b1"), ("group", ["w:a1", "w:a2", "w:b1"]),
                   ("A", "got", ["y:xa1", "y:xa2"]), ("B", "got", "y:xb1"),
                   ("A", "call", "a3"), ("B", "call", "b2"), ("B", "call", "b3"), ("group", ["w:a3", "w:b2", "w:b3"]),
                   ("A", "got", "y:xa3"), ("B", "got", ["y:xb2", "y:xb3"])]
    assert res == (("ra", [["y:xa1", "y:xa2"], "y:xa3"]), ("rb", ["y:xb1", ["y:xb2", "y:xb3"]]))


def test_two_list_requests_share_one_launch(log):
    res = _run(log, [[R("a1"), R("a2")]], [[R("b1")]])
    assert log == [("A", "call", "a1"), ("A", "call", "a2"), ("B", "call", "b1"), ("group", ["w:a1", "w:a2", "w:b1"]),
                   ("A", "got", ["y:xa1", "y:xa2"]), ("B", "got", ["y:xb1"])]
    assert res == (("ra", [["y:xa1", "y:xa2"]]), ("rb", [["y:xb1"]]))


@pytest.mark.parametrize("who", ["A", "B"])
def test_a_request_with_pre_is_not_grouped(log, who):
    """a pair launch has no group form: both engines serve their own request, A first, and both answers arrive after both launches"""
    pre = dict(pre=("x2", "a0"))
    res = _run(log, [R("a1", **(pre if who == "A" else {})), R("a2")], [R("b1", **(pre if who == "B" else {})), R("b2")])
    assert log == [("A", "serve", "a1"), ("B", "serve", "b1"), ("A", "got", "y:xa1"), ("B", "got", "y:xb1"),
                   ("A", "call", "a2"), ("B", "call", "b2"), ("group", ["w:a2", "w:b2"]), ("A", "got", "y:xa2"), ("B", "got", "y:xb2")]
    assert res == (("ra", ["y:xa1", "y:xa2"]), ("rb", ["y:xb1", "y:xb2"]))


def test_pre_inside_a_list_request_does_not_stop_the_grouping(log):
    """the exception looks at single requests only (a list request never carries `pre`: the group launch has no such form)"""
    res = _run(log, [[R("a1", pre=None)]], [R("b1")])
    assert log == [("A", "call", "a1"), ("B", "call", "b1"), ("group", ["w:a1", "w:b1"]), ("A", "got", ["y:xa1"]), ("B", "got", "y:xb1")]
    assert res == (("ra", [["y:xa1"]]), ("rb", ["y:xb1"]))


def test_a_generator_that_returns_at_once(log):
    res = _run(log, [], [R("b1"), R("b2")])
    assert log == [("B", "serve", "b1"), ("B", "got", "y:xb1"), ("B", "serve", "b2"), ("B", "got", "y:xb2")]
    assert res == (("ra", []), ("rb", ["y:xb1", "y:xb2"]))
    del log[:]
    assert _run(log, [R("a1")], []) == (("ra", ["y:xa1"]), ("rb", []))
    assert log == [("A", "serve", "a1"), ("A", "got", "y:xa1")]
    del log[:]
    assert _run(log, [], []) == (("ra", []), ("rb", [])) and log == []


def test_streams_alternate_strictly_and_never_group(log, monkeypatch):
    """streams = (s, s): every launch and every resumption of a generator inside its own model's stream context, A and B in turn, no grouped
    launch and no `_conv_call` -- also for a request the plain mode would have grouped"""
    made = []

    class Scope:
        def __init__(self, stream):
            self.i = len(made)
            made.append(stream)

        def __enter__(self):
            log.append(("enter", self.i))

        def __exit__(self, *exc):
            log.append(("exit", self.i))
            return False
    monkeypatch.setattr(torch.cuda, "stream", Scope)
    s = object()
    res = _run(log, [R("a1"), [R("a2"), R("a3")], R("a4")], [R("b1"), R("b2", pre=("x2", "b0"))], streams=(s, s))
    assert made == [s, s]
    assert log == [("enter", 0), ("exit", 0), ("enter", 1), ("exit", 1),
                   ("enter", 0), ("A", "serve", "a1"), ("A", "got", "y:xa1"), ("exit", 0),
                   ("enter", 1), ("B", "serve", "b1"), ("B", "got", "y:xb1"), ("exit", 1),
                   ("enter", 0), ("A", "serve", ["a2", "a3"]), ("A", "got", ["y:xa2", "y:xa3"]), ("exit", 0),
                   ("enter", 1), ("B", "serve", "b2"), ("B", "got", "y:xb2"), ("exit", 1),
                   ("enter", 0), ("A", "serve", "a4"), ("A", "got", "y:xa4"), ("exit", 0)]
    assert res == (("ra", ["y:xa1", ["y:xa2", "y:xa3"], "y:xa4"]), ("rb", ["y:xb1", "y:xb2"]))
