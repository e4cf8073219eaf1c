"""Priorities answers prepared behind their filter's answer, plan memos re-validated ahead.

A front-door worker computes the priorities answer of the pod it just filtered in the spin
window behind that filter's answer (Frontend::prepare_priorities) and hands it out when the
priorities request arrives and everything the answer depends on still reads the same; anything
else takes the verb's own path. Either way the body is the Python verb's, byte for byte, on the
ledger state of its moment. The second half: after a nomination, the nominated node's plan
memos are re-validated in the spin window, so the next filter runs no scan and no
re-validation of its own (Frontend::memo_ahead_step).

A started front door is driven over its socket on one keep-alive connection, as kube-scheduler
drives it; 3 nodes x 2 GPUs and one-container pods are the smallest shapes with a tie, a node
that does not fit and a lead.
"""
from __future__ import annotations

import json
import select
import socket
import time

import pytest

from nanogpu import _native as N
from nanogpu.extender.verbs import Extender
from nanogpu.k8s import podutil as pu
from nanogpu.k8s.fake_apiserver import FakeKubeStore, InProcKube
from nanogpu.state.cluster import ClusterState
from nanogpu.topology.model import synthetic_mi355x

NAMES = ["n0", "n1", "n2"]
COUNTERS = ("prio_prepared", "prio_prepared_used", "prio_prepared_stale")


def _dumps(o) -> bytes:
    return json.dumps(o, separators=(",", ":")).encode()


def _args(pod, names) -> bytes:
    return _dumps({"Pod": pod, "Nodes": None, "NodeNames": names})


def _pod(name, pct=50, owner=None):
    pod = pu.make_pod(name, [("c", pct)], uid=f"uid-{name}")
    if owner:
        pod["metadata"]["ownerReferences"] = [
            {"apiVersion": "apps/v1", "kind": "ReplicaSet", "name": "rs", "uid": owner, "controller": True}]
    return pod


class _Conn:
    """One keep-alive connection; a request is sent and its answer read before the next."""

    def __init__(self, port: int):
        self.s = socket.create_connection(("127.0.0.1", port))
        self.s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        self.s.settimeout(10)
        self.buf = b""

    def send(self, path: str, body: bytes) -> None:
        self.s.sendall(f"POST {path} HTTP/1.1\r\nHost: x\r\nContent-Length: {len(body)}\r\n\r\n".encode() + body)

    def read(self) -> bytes:
        while b"\r\n\r\n" not in self.buf:
            self.buf += self.s.recv(65536)
        head, _, rest = self.buf.partition(b"\r\n\r\n")
        assert head.split(b" ")[1] == b"200", head
        clen = int([h.split(b":")[1] for h in head.split(b"\r\n") if h.lower().startswith(b"content-length")][0])
        while len(rest) < clen:
            rest += self.s.recv(65536)
        self.buf = rest[clen:]
        return rest[:clen]

    def post(self, path: str, body: bytes) -> bytes:
        self.send(path, body)
        return self.read()

    def close(self) -> None:
        self.s.close()


class _Door:
    """A cluster of 3 nodes x 2 GPUs, the Python verbs over it, and a started front door with
    one worker on the same ledger, under the Python verbs' rules."""

    def __init__(self, normalize=False, lead=100, decisive=False, learn_sizes=True):
        self.st = ClusterState(nominate=True, score_normalize=normalize, priority_lead=lead,
                               decisive_filter=decisive, learn_sizes=learn_sizes)
        for n in NAMES:
            self.st.register_node(pu.make_node(n, 2, synthetic_mi355x(2).to_json()))
        self.led = self.st.ledger
        self.ext = Extender(self.st, InProcKube(FakeKubeStore()))
        self.fe = N.Frontend(self.led, "127.0.0.1", 0, 1)
        self.set_options()
        self.c = _Conn(self.fe.port)
        self.n = 0

    def set_options(self):
        st = self.st
        self.fe.set_options(st.options, st.score_normalize, st.nominate, st.decisive_filter, st.priority_lead)

    def fill(self, node: str, pct: int):
        self.n += 1
        rc = self.led.reserve(self.led.find_node(node), f"base-{self.n}", [(pct, 0)], self.st.options)
        assert rc[0] == N.OK, rc

    def counters(self):
        s = self.fe.stats()
        return tuple(s[k] for k in COUNTERS)

    def filter(self, pod, names) -> list[str]:
        """The native filter; its body is the Python verb's (which changes nothing while more
        than one node fits). Returns the fitting nodes: the list priorities is sent."""
        raw = _args(pod, names)
        out = self.c.post("/scheduler/filter", raw)
        assert out == _dumps(self.ext.filter(json.loads(raw)))
        return json.loads(out)["NodeNames"]

    def priorities(self, pod, names) -> bytes:
        """The native priorities answer, checked against the Python verb's on the same state:
        the same bytes, and the same node nominated (or none)."""
        raw = _args(pod, names)
        out = self.c.post("/scheduler/priorities", raw)
        assert self.led.wait_deferred_nominations(5_000_000_000)   # made behind the answer
        mine = self.led.lookup(pu.pod_uid(pod))
        assert out == _dumps(self.ext.prioritize(json.loads(raw)))
        theirs = self.led.lookup(pu.pod_uid(pod))   # Python dropped the nomination and made its own
        assert (mine and (mine["state"], mine["node"])) == (theirs and (theirs["state"], theirs["node"]))
        return out

    def close(self):
        self.c.close()
        self.fe.stop()


@pytest.fixture
def door(request):
    d = _Door(**getattr(request, "param", {}))
    yield d
    d.close()


def _delta(d, before):
    return tuple(a - b for a, b in zip(d.counters(), before))


# ------------------------------------------------------------------ taken as prepared
def _setup_unique(d):          # every node fits, n0 is the unique best (binpack: the fuller device)
    d.fill("n0", 50)
    d.fill("n1", 25)
    return NAMES


def _setup_one_unfit(d):       # n2 is full: priorities is sent the fitting subset
    d.fill("n2", 100)
    d.fill("n2", 100)
    d.fill("n0", 25)
    return NAMES


def _setup_tie(d):             # three identical nodes: a tie at the top, broken by the UID hash, then led
    return NAMES


@pytest.mark.parametrize("door,setup", [
    ({}, _setup_unique),
    ({}, _setup_one_unfit),
    ({}, _setup_tie),
    ({"normalize": True}, _setup_unique),
    ({"normalize": True}, _setup_tie),
    ({"lead": 0}, _setup_unique),
    ({"lead": 0}, _setup_tie),
], indirect=["door"], ids=["all_fit", "one_unfit", "tie", "normalize", "normalize_tie", "lead0", "lead0_tie"])
def test_the_prepared_answer_is_taken_and_is_the_python_verbs(door, setup):
    names = setup(door)
    for k in range(3):   # each pod's nomination changes the nodes the next one sees
        pod = _pod(f"p{k}")
        before = door.counters()
        fit = door.filter(pod, names)
        assert len(fit) > 1 and (len(fit) < len(names)) == (setup is _setup_one_unfit)
        out = door.priorities(pod, fit)
        assert _delta(door, before) == (1, 1, 0)
        scores = [h["Score"] for h in json.loads(out)]
        rec = door.led.lookup(pu.pod_uid(pod))
        assert rec["state"] == "nominated"     # every case here has a winner, tie-broken or unique
        best = scores.index(max(scores))
        assert door.led.find_node(fit[best]) == rec["node"] and scores.count(max(scores)) == 1
        if door.st.priority_lead and not door.st.score_normalize:
            assert max(scores) - sorted(scores)[-2] >= door.st.priority_lead
        door.led.drop_nomination(pu.pod_uid(pod))
        door.fill(fit[best], 50)     # the pod's bind, as far as the next pod can tell


# ------------------------------------------------------------------ not taken
def _reserve_release(d, pod, fit):
    nid = d.led.find_node(fit[0])
    assert d.led.reserve(nid, "other", [(25, 0)], d.st.options)[0] == N.OK
    d.led.release("other")
    assert d.led.lookup("other") is None
    return fit


def _reserve(d, pod, fit):     # (stays: the fresh answer differs from the prepared one)
    assert d.led.reserve(d.led.find_node(fit[0]), "other", [(50, 0)], d.st.options)[0] == N.OK
    return fit


def _nominate_other(d, pod, fit):
    d.led.nominate(d.led.find_node(fit[-1]), "other", [(50, 0)], d.st.options)
    return fit


def _set_options(d, pod, fit):
    d.st.score_normalize = True
    d.set_options()
    return fit


def _raise_margin(d, pod, fit):
    # a pod bound elsewhere than its nomination raises the margin (Ledger::reserve)
    m0 = d.led.nomination_margin
    d.led.nominate(d.led.find_node(fit[0]), "moved", [(25, 0)], d.st.options)
    assert d.led.reserve(d.led.find_node(fit[1]), "moved", [(25, 0)], d.st.options)[0] == N.OK
    assert d.led.nomination_margin > m0
    return fit


def _owner_streams(d, pod, fit):
    d.led.set_stream_owner("rs-1", True)    # the pod's demand turns memory-bound: nothing else moves
    return fit


def _other_pods_filter(d, pod, fit):
    d.filter(_pod("q", 25), NAMES)
    return fit


def _reordered(d, pod, fit):
    return fit[::-1]


def _one_fewer(d, pod, fit):
    return fit[:-1]


@pytest.mark.parametrize("between", [_reserve_release, _reserve, _nominate_other, _set_options, _raise_margin,
                                     _owner_streams, _other_pods_filter, _reordered, _one_fewer])
@pytest.mark.parametrize("setup", [_setup_unique, _setup_one_unfit], ids=["all_fit", "one_unfit"])
def test_a_prepared_answer_out_of_date_is_not_taken(door, setup, between):
    names = setup(door)
    pod = _pod("p0", owner="rs-1")
    before = door.counters()
    fit = door.filter(pod, names)
    sent = between(door, pod, fit)
    door.priorities(pod, sent)     # the Python verb's bytes on the state of this moment
    prepared, used, stale = _delta(door, before)
    # (another pod's filter prepares an answer of its own: two prepared, the second one found stale)
    assert used == 0 and stale == 1 and prepared == (2 if between is _other_pods_filter else 1)


def test_a_prepared_answer_is_used_once(door):
    door.fill("n0", 50)
    pod = _pod("p0")
    fit = door.filter(pod, NAMES)
    before = door.counters()
    first = door.priorities(pod, fit)
    assert _delta(door, before) == (0, 1, 0)
    door.led.drop_nomination(pu.pod_uid(pod))
    before = door.counters()
    assert door.priorities(pod, fit) == first      # computed: nothing is prepared any more
    assert _delta(door, before) == (0, 0, 0)


@pytest.mark.parametrize("door", [{}, {"decisive": True}], indirect=True, ids=["one_fits", "decisive"])
def test_nothing_is_prepared_when_no_priorities_call_follows(door):
    if not door.st.decisive_filter:
        for n in ("n1", "n2"):
            door.fill(n, 100)
            door.fill(n, 100)
    pod = _pod("p0")
    raw = _args(pod, NAMES)
    out = door.c.post("/scheduler/filter", raw)
    (only,) = json.loads(out)["NodeNames"]      # the one that fits, or the decisive filter's pick
    assert door.led.wait_deferred_nominations(5_000_000_000)
    assert door.led.lookup(pu.pod_uid(pod))["state"] == "nominated"    # the filter's own nomination
    door.led.drop_nomination(pu.pod_uid(pod))
    before = door.counters()
    door.priorities(pod, [only])       # a scheduler that asks all the same: computed
    assert door.counters() == before == (0, 0, 0)


# ------------------------------------------------------------------ the switch, and the memos ahead
def _cycles(monkeypatch, switch):
    """Five pods of two demand classes through filter, priorities and bind on a busy-polling
    front door. Returns every body, the ledger work the filters did themselves (scans,
    re-validations and full evaluations counted while a filter was on the wire) per pod, and the
    counters at the end.

    Request sizes are not learned here: a newly learned size changes the options' hash, which
    starts every class's memos afresh (with or without this switch), so the second class's first
    pod would make the first class new again."""
    if switch is None:
        monkeypatch.delenv("NANOGPU_FE_PREPARE", raising=False)
    else:
        monkeypatch.setenv("NANOGPU_FE_PREPARE", switch)
    d = _Door(learn_sizes=False)
    bind_c = _Conn(d.fe.port)
    d.fe.set_busy_poll_us(20_000)
    d.fe.set_spin_recv(True)
    N.io_tally_reset()
    N.io_tally_enable(True)

    def ledger_work():
        t = N.io_tally()
        return sum(t.get(k, (0, 0))[0] for k in ("ledger_scan", "ledger_revalidate", "ledger_choose"))

    bodies, work, ahead = [], [], 0
    try:
        for k, pct in enumerate([50, 25, 50, 25, 50]):
            pod = _pod(f"p{k}", pct)
            w0 = ledger_work()
            out = d.c.post("/scheduler/filter", _args(pod, NAMES))
            work.append(ledger_work() - w0)
            bodies.append(out)
            fit = json.loads(out)["NodeNames"]
            assert fit == NAMES
            out = d.c.post("/scheduler/priorities", _args(pod, fit))
            bodies.append(out)
            assert d.led.wait_deferred_nominations(5_000_000_000)
            scores = [h["Score"] for h in json.loads(out)]
            node = fit[scores.index(max(scores))]
            rec = d.led.lookup(pu.pod_uid(pod))
            assert rec["state"] == "nominated" and rec["node"] == d.led.find_node(node)
            if switch in (None, "1", "b"):
                # the nominated node's memos, one per class seen so far, are brought up to date
                # in the spin window behind the priorities answer: waited for, not slept for
                ahead += min(k + 1, 2)
                t_end = time.monotonic() + 5
                while d.fe.stats()["memo_ahead"] < ahead and time.monotonic() < t_end:
                    time.sleep(0.0002)
                assert d.fe.stats()["memo_ahead"] == ahead
            bind_c.send("/scheduler/bind", _dumps({"PodName": f"p{k}", "PodNamespace": "default",
                                                    "PodUID": pu.pod_uid(pod), "Node": node}))
            assert select.select([d.fe.notify_fd()], [], [], 5)[0]
            (req,) = d.fe.take()       # reserved natively (the nomination adopted); Python's half: the writes
            assert d.led.lookup(pu.pod_uid(pod))["state"] == "reserved"
            d.fe.respond(req[0], 200, "application/json", b'{"Error":""}')
            assert bind_c.read() == b'{"Error":""}'
        return bodies, work, d.fe.stats()
    finally:
        N.io_tally_enable(False)
        bind_c.close()
        d.close()


def test_memos_are_revalidated_ahead_of_the_filter_and_no_answer_changes(monkeypatch):
    off_bodies, off_work, off = _cycles(monkeypatch, "0")
    on_bodies, on_work, on = _cycles(monkeypatch, None)
    assert on_bodies == off_bodies
    # after the first cycle of each class (pods 0 and 1) a filter does no ledger work of its own
    assert on_work[2:] == [0, 0, 0], on_work
    assert all(w > 0 for w in off_work[2:]), off_work     # which it pays for with the switch off
    assert on["memo_ahead"] == 1 + 2 * 4 and off["memo_ahead"] == 0
    assert [off[k] for k in COUNTERS] == [0, 0, 0]
    assert [on[k] for k in COUNTERS] == [5, 5, 0]


@pytest.mark.parametrize("switch,prepared,ahead", [("0", False, False), ("a", True, False), ("b", False, True),
                                                    ("1", True, True)])
def test_the_switch_turns_each_half_on_alone(monkeypatch, switch, prepared, ahead):
    _, _, s = _cycles(monkeypatch, switch)
    assert [s[k] for k in COUNTERS] == ([5, 5, 0] if prepared else [0, 0, 0])
    assert (s["memo_ahead"] > 0) == ahead
