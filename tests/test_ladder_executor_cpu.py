"""CPU: the precision ladder's executor (hip_ext.engine.DepthEngine._ladder) over stand-in rungs -- no GPU, no library call.  The three rungs are fakes whose output
names the rung and the image (1000 * rung + image), the two reductions are fakes that report a prescribed r / diversity per (image, rung); the control flow, the
index bookkeeping and the counters are the real ones.  Checked: whichever rung runs first, every image carries the output of the rung the first-rung-first rule
assigns it, the counters and the next start rung follow from that rung vector, and nothing is run that is not needed."""
import random
import warnings
from types import SimpleNamespace

import pytest
import torch

import hip_ext.engine as E
from hip_ext.ladder import ladder_decide, next_start_rung

D = 64
THR, THR3 = 0.4, 0.6


class _FakeWS:
    """The fields of a Workspace that the ladder reads; taps[3] / a_pe carry (image, which engine) instead of features."""

    def __init__(self, B, engine_index):
        self.B, self.H, self.W, self.ph, self.pw = B, 14, 14, 1, 1
        self.engine_index = engine_index
        self.taps = [None, None, None, torch.zeros(B, 2)]
        self.a_pe = torch.zeros(B, 3)
        self.stat_buf = torch.zeros(B * (E.STAT_CHUNKS + 2) * 2)
        self.stat_sums = self.stat_buf[:B * E.STAT_CHUNKS * 2].view(B, E.STAT_CHUNKS, 2)
        self.stat_div = self.stat_buf[B * E.STAT_CHUNKS * 2:B * (E.STAT_CHUNKS + 1) * 2].view(B, 1, 2)
        self.stat_in = self.stat_buf[B * (E.STAT_CHUNKS + 1) * 2:].view(B, 1, 2)

    def load(self, x):
        for t in (self.taps[3], self.a_pe):
            t[:, 0] = x.flatten(1)[:, 0]
            t[:, 1] = self.engine_index


def _out(ids, rung):
    return (ids.double() + 1000 * rung).view(-1, 1, 1, 1).repeat(1, 1, 14, 14).clone()


@pytest.fixture
def rig(monkeypatch):
    """(make_engine, table, log): table[image] = dict(r={rung: r}, div=[first rung's, third's], din=[...]) is what the fake reductions report."""
    table, log = {}, []

    def depth_stats(out, sums, act):
        sums.zero_()
        for b in range(out.shape[0]):
            v = int(out[b].flatten()[0])
            sums[b, 0, 0], sums[b, 0, 1] = 1.0, table[v % 1000]["r"][v // 1000]

    def token_diversity(tap, ld, B, rows, dim, stat):
        stat.zero_()
        key = "div" if tap.shape[1] == 2 else "din"
        for b in range(B):
            stat[b, 0, 0], stat[b, 0, 1] = table[int(tap[b, 0])][key][int(tap[b, 1])], 1.0
    monkeypatch.setattr(E, "k_depth_stats", depth_stats)
    monkeypatch.setattr(E, "k_token_diversity", token_diversity)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)

    class Third:
        def __init__(self):
            self.w, self.final_act, self._ws = SimpleNamespace(dim=D, pe_seg=64), 1, {}

        def workspace(self, B, H, W, dev):
            return self._ws.setdefault(B, _FakeWS(B, 1))

        def forward(self, x, guide, norm):
            self.workspace(x.shape[0], 14, 14, x.device).load(x)
            log.append(("third", x.flatten(1)[:, 0].int().tolist()))
            return _out(x.flatten(1)[:, 0], 3)

    def make_engine(kind):
        hi = SimpleNamespace()
        lad = {"full": dict(r=THR, r3=THR3, div=0.1, div_in=1e-4, make=lambda: hi, make3=Third),
               "no third": dict(r=THR, div=0.1, div_in=1e-4, make=lambda: hi),
               "third only": dict(div_in=1e-4, make3=Third, r3=THR3)}[kind]
        eng = object.__new__(E.DepthEngine)
        eng.w, eng.final_act, eng.ladder = SimpleNamespace(dim=D, pe_seg=64), 1, lad
        eng._warned, eng._start_rung, eng._w_hi, eng._eng3 = False, 1, None, None
        eng.second_rung_first_calls = eng.third_rung_first_calls = eng.escalated = eng.escalated3 = 0
        eng.last_ratio = eng.last_diversity = eng.last_input_diversity = None
        wss = {}

        def workspace(B, H, W, dev):
            return wss.setdefault(B, _FakeWS(B, 0))

        def forward(x, guide, norm=None, head=True):
            ws = workspace(x.shape[0], 14, 14, x.device)
            ws.load(x)
            log.append(("encoder + first head" if head else "encoder", x.flatten(1)[:, 0].int().tolist()))
            return _out(x.flatten(1)[:, 0], 1) if head else ws

        def head_for(ws, B, idx, w):
            ids = ws.taps[3][:, 0] if idx is None else ws.taps[3][:, 0][idx]
            log.append(("first head" if w is eng.w else "second head", ids.int().tolist()))
            return _out(ids, 1 if w is eng.w else 2)
        eng.workspace, eng._forward, eng._head_for = workspace, forward, head_for
        return eng
    return make_engine, table, log


# r of an image on the first rung: clear of the thresholds, or so close that a higher rung's r (within 1e-3 of it) lands in the guard band / on the other side
POINTS = [0.1, 0.39, THR * 0.9995, THR * 1.0005, THR * 1.015, 0.45, 0.5, THR3 * 0.985, THR3 * 0.9995, THR3 * 1.0005, THR3 * 1.015, THR3 * 1.03, 0.7, 0.9]


@pytest.mark.parametrize("kind", ["full", "no third", "third only"])
def test_every_image_carries_its_rung_whichever_rung_runs_first(rig, kind):
    make_engine, table, log = rig
    rnd = random.Random(11)
    calls = {1: 0, 2: 0, 3: 0}
    mixed = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for trial in range(150):
            eng = make_engine(kind)
            lad = eng.ladder
            for _ in range(4):
                B = rnd.choice([1, 2, 3, 5, 8])
                table.clear()
                pts = [rnd.choice(POINTS)] if rnd.random() < 0.4 else POINTS        # a stream of like images, or a mixed batch
                for i in range(B):
                    r1 = rnd.choice(pts)
                    flat = rnd.random() < 0.15
                    by_tap = flat and rnd.random() < 0.5
                    table[i] = dict(r={1: r1, 2: r1 * (1 + rnd.uniform(-1e-3, 1e-3)), 3: r1 * (1 + rnd.uniform(-1e-3, 1e-3))},
                                    div=[0.01 if by_tap else 0.3] * 2, din=[1e-6 if flat and not by_tap else 0.2] * 2)
                if rnd.random() < 0.25:
                    eng._start_rung = rnd.choice([1, 2, 3])
                asked = eng._start_rung
                start = 3 if (asked == 3 and "make3" in lad) else 2 if (asked == 2 and "make" in lad) else 1      # (a start rung that cannot be honoured: the first)
                before = (eng.escalated, eng.escalated3, eng.second_rung_first_calls, eng.third_rung_first_calls)
                x = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1).repeat(1, 3, 14, 14)
                del log[:]
                out = eng._ladder(x, None, None)
                # the yardstick: the first-rung-first rule on the image's own first-rung statistics
                r1 = torch.tensor([table[i]["r"][1] for i in range(B)], dtype=torch.float64)
                flat = torch.tensor([table[i]["div"][0] < lad.get("div", 0.0) or table[i]["din"][0] < 1e-4 for i in range(B)])
                want = ladder_decide(r1, flat, lad, 1, E.LADDER_GUARD)
                assert out.flatten(1)[:, 0].tolist() == [1000.0 * int(k) + i for i, k in enumerate(want)], (kind, start, table, log)
                assert bool((out.flatten(1) == out.flatten(1)[:, :1]).all())
                after = (eng.escalated, eng.escalated3, eng.second_rung_first_calls, eng.third_rung_first_calls)
                assert tuple(a - b for a, b in zip(after, before)) == (int((want >= 2).sum()), int((want == 3).sum()), int(start == 2), int(start == 3))
                assert eng._start_rung == next_start_rung(want, "make" in lad)
                # r: the first rung's wherever it ran for the image, else the start rung's; the diversities always one per image
                ran_first = set(range(B)) if start == 1 else {i for name, ids in log if name in ("first head", "encoder + first head") for i in ids}
                f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))     # noqa: E731  (the statistics buffer is fp32)
                assert eng.last_ratio.tolist() == [f32(table[i]["r"][1 if i in ran_first else start]) for i in range(B)]
                assert len(eng.last_input_diversity) == B and (eng.last_diversity is None) == ("div" not in lad)
                # nothing twice, except the third rung for an undecided image behind the third rung; the encoder of this engine at most once per image
                runs = [(name, i) for name, ids in log for i in ids]
                again = {(n, i) for n, i in runs if runs.count((n, i)) > 1}
                assert all(n == "third" and start == 3 and i in ran_first for n, i in again), (start, log)
                assert {i for n, i in runs if n == "second head"} == ({i for i in range(B) if want[i] == 2} if start != 2 else set(range(B)))
                calls[start] += 1
                mixed += len(set(want.tolist())) > 1 and start != 1
    assert kind != "full" or (min(calls.values()) > 20 and mixed > 20)


def test_no_ladder_and_warning_once(rig):
    make_engine, table, log = rig
    eng = make_engine("full")
    table[0] = dict(r={1: 0.5, 2: 0.5, 3: 0.5}, div=[0.3, 0.3], din=[0.2, 0.2])
    x = torch.zeros(1, 3, 14, 14)
    with pytest.warns(UserWarning, match="precision ladder: 1 of 1"):
        eng._ladder(x, None, None)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng._ladder(x, None, None)                      # second rung first now: the one warning covers every order
    assert eng.second_rung_first_calls == 1 and eng.escalated == 2
    eng.ladder = None
    assert eng._ladder(x, None, None).flatten()[0] == 1000.0 and eng.escalated == 2
