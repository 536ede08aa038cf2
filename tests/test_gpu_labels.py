"""Triple-barrier labels and sample weights on the MI355X against the reference's recorded outputs (tests/golden/labels.npz) and,
bit for bit, against the NumPy restatement of tests/_label_ref.py."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from tests import _counts
from tests import _label_ref as H
from tests.test_labels_host import CASES, rel_close

pytestmark = pytest.mark.gpu

BLOCK = 1024            # ticks per entry of the long schedule's table (csrc/fmk_label.hip)


def diag_last(ctx):
    from finmlkit_amd import _ffi
    out = (C.c_int64 * 5)()
    _ffi.check(_ffi.lib().fmk_diag_label_last(ctx.handle, out), ctx.handle)
    return dict(zip(("schedule", "events", "skipped", "opened", "walked"), list(out)))


class forced:
    """FMK_LABEL_SCHEDULE for the duration of a block (None: the library's own choice)."""

    def __init__(self, schedule):
        self.schedule = schedule

    def __enter__(self):
        self.old = os.environ.pop("FMK_LABEL_SCHEDULE", None)
        if self.schedule:
            os.environ["FMK_LABEL_SCHEDULE"] = self.schedule

    def __exit__(self, *a):
        os.environ.pop("FMK_LABEL_SCHEDULE", None)
        if self.old is not None:
            os.environ["FMK_LABEL_SCHEDULE"] = self.old


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, what
    assert np.array_equal(got.view(np.uint8 if got.dtype.itemsize == 1 else "u%d" % got.dtype.itemsize),
                          want.view(np.uint8 if want.dtype.itemsize == 1 else "u%d" % want.dtype.itemsize)) or \
        np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), what


def check_tb_bits(ts, px, ev, tg, hb, vb, mc, side, min_ret, schedule, lc=None, name=None, max_skipped_pct=1.0):
    """All four outputs bit for bit against the helper, every event; -> (helper outputs, events skipped)."""
    from finmlkit_amd import _ffi, label
    want = H.triple_barrier(ts, px, ev, tg, hb, vb, mc, side, min_ret, log_close=lc)
    with forced(schedule):
        got = label.triple_barrier(ts, px, ev, tg, hb, vb, mc, side, min_ret)
    d = diag_last(_ffi.default_context())
    skipped = want[4]
    assert d["skipped"] == skipped.sum() and d["events"] == len(ev)
    if schedule:
        assert d["schedule"] == (schedule == "long")
    assert skipped.sum() * 100 <= max_skipped_pct * len(ev)
    for g, w, what in zip(got, want[:4], ("labels", "touch_idx", "returns", "ratios")):
        assert_bits(g, w, f"{name}/{schedule}/{what}")
    if name:
        _counts.record(f"labels/{name}/{schedule or 'default'}", events_compared=len(ev), events_skipped=int(skipped.sum()))
    return want, d


# ---------------------------------------------------------------------------------------------- fixtures of the reference
@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_functions_vs_reference(orc, name):
    from finmlkit_amd import label
    c = CASES[name]
    ts, px, _, _ = orc.synth(c["seed"], 0, c["n"])
    lab, tch, ret, rat = label.triple_barrier(ts, px, c["event_idx"], c["targets"], c["hb"], c["vb"], c["mc"], c["side"],
                                              c["min_ret"])
    ok = ~c["skipped"]
    assert ok.sum() * 100 > 99 * len(ok)
    assert lab.dtype == np.int8 and tch.dtype == np.int64
    assert np.array_equal(lab[ok], c["labels"][ok]) and np.array_equal(tch[ok], c["touch_idx"][ok])
    assert np.array_equal(tch[~ok], c["event_idx"][~ok])
    tol = 4 * 2.0 ** -52 * np.abs(np.log(px)).max()
    d = np.abs(ret[ok] - c["returns"][ok]).max()
    print(name, "max |ret - ref| =", d, "tol", tol)
    assert d <= tol
    assert rel_close(rat[ok], c["ratios"][ok], 1e-12)
    avg, conc = label.average_uniqueness(ts, c["event_idx"], c["touch_idx"])
    assert conc.dtype == np.int16 and np.array_equal(conc, c["concurrency"])
    print(name, "avg uniqueness max rel", np.max(np.abs(avg - c["avg_uniqueness"]) / c["avg_uniqueness"]))
    assert rel_close(avg, c["avg_uniqueness"], 1e-9)
    _, bound = H.return_attribution(c["event_idx"], c["touch_idx"], px, conc, False)
    att = label.return_attribution(c["event_idx"], c["touch_idx"], px, conc, False)
    print(name, "attribution max err / bound", np.max(np.abs(att - c["return_attribution"]) / np.maximum(bound, 1e-300)))
    assert np.all(np.abs(att - c["return_attribution"]) <= bound)
    attn = label.return_attribution(c["event_idx"], c["touch_idx"], px, conc, True)
    scale = len(att) / c["return_attribution"].sum()
    assert np.all(np.abs(attn - c["return_attribution_norm"]) <= bound * scale + 1e-12 * attn)
    assert abs(attn.sum() - len(attn)) <= 1e-9 * len(attn)
    _counts.record(f"labels/reference/{name}", events_compared=int(ok.sum()), events_skipped=int((~ok).sum()))


@pytest.mark.parametrize("name", ["symmetric", "meta"])
def test_kit_frames_vs_reference(orc, name):
    from finmlkit_amd.bar.data_model import TradesData
    from finmlkit_amd.label import SampleWeights, TBMLabel
    c = CASES[name]
    ts, px, am, _ = orc.synth(c["seed"], 0, c["n"])
    trades = TradesData(ts, px, am.astype(np.float64), np.arange(c["n"]), dt_index=pd.to_datetime(ts))
    order = np.argsort(c["event_idx"], kind="stable")
    ev = c["event_idx"][order]
    feats = pd.DataFrame({"event_idx": ev, "sigma": c["targets"][order]}, index=pd.to_datetime(ts[ev]))
    if c["side"] is not None:
        feats["side"] = c["side"][order].astype(np.int64)
    tbm = TBMLabel(feats, "sigma", c["min_ret"], c["hb"], pd.Timedelta(seconds=c["vb"]),
                   min_close_time=pd.Timedelta(seconds=c["mc"]), is_meta=c["side"] is not None)
    f, out = tbm.compute_labels(trades)
    assert len(f) == len(ev) and f.index.equals(feats.index) and out.index.equals(feats.index)
    assert list(out.columns) == ["touch_time", "event_idx", "touch_idx", "labels", "returns", "vertical_touch_weights"]
    assert out["labels"].dtype == np.int8 and out["touch_idx"].dtype == np.int64 and out["returns"].dtype == np.float64
    assert str(out["touch_time"].dtype).startswith("datetime64[ns")
    assert np.array_equal(out["labels"].values, c["labels"][order])
    assert np.array_equal(out["touch_idx"].values, c["touch_idx"][order])
    assert np.array_equal(out["touch_time"].values.astype(np.int64), ts[c["touch_idx"][order]])
    assert rel_close(out["vertical_touch_weights"].values, c["ratios"][order], 1e-12)
    assert tbm._tape is not None and tbm._tape_of is trades
    w = tbm.compute_weights(trades)
    assert tbm._tape is None                                               # the resident copy is released after use
    w2 = SampleWeights.compute_info_weights(trades, out)                   # the NumPy-level route: same numbers
    assert list(w.columns) == ["avg_uniqueness", "return_attribution"] and w.index.equals(out.index)
    assert rel_close(w["avg_uniqueness"].values, c["avg_uniqueness"][order], 1e-9)
    assert np.array_equal(w.values, w2.values)
    _, bound = H.return_attribution(ev, c["touch_idx"][order], px, c["concurrency"], False)
    assert np.all(np.abs(w["return_attribution"].values - c["return_attribution"][order]) <= bound)
    fin = SampleWeights.compute_final_weights(w["avg_uniqueness"], 0.5, w["return_attribution"], out["vertical_touch_weights"],
                                              out["labels"])
    assert list(fin.columns) == ["time_decay_weights", "return_attribution", "vertical_touch_weights", "weights"]
    assert abs(fin["return_attribution"].sum() - len(fin)) < 1e-6
    _counts.record(f"labels/kit/{name}", events_compared=len(ev), events_skipped=0)


# ---------------------------------------------------------------------------------------------- bit for bit against the helper
@pytest.fixture(scope="module")
def tape(orc):
    n = 1_000_000
    ts, px, _, _ = orc.synth(77, 0, n)
    return ts, px, H.log_column(px)


def _sigma(lc, w):
    return float(np.std(lc[w:] - lc[:-w]))


@pytest.mark.parametrize("schedule", ["direct", "long", None])
def test_bits_on_a_million_ticks(tape, schedule):
    ts, px, lc = tape
    n = len(ts)
    rng = np.random.default_rng(5)
    last = int(np.searchsorted(ts, ts[-1] - 600 * 10 ** 9)) - 1
    ev = np.concatenate([[0], rng.choice(np.arange(1, last), 2998, replace=False), [n - 2]]).astype(np.int64)
    rng.shuffle(ev)
    tg = _sigma(lc, 1200) * (0.25 + 2 * rng.random(len(ev)))
    sd = rng.integers(-1, 2, len(ev)).astype(np.int8)
    for k, (hb, vb, mc, side, mr) in enumerate([((1.0, 1.0), 60.0, 1.0, None, 0.0), ((1.0, 2.0), 600.0, 0.0, sd, 1e-5),
                                                ((np.inf, 1.0), 60.0, 2.5, None, 0.0), ((0.0, 0.0), 30.0, 1.0, None, 0.0)]):
        check_tb_bits(ts, px, ev, tg, hb, vb, mc, side, mr, schedule, lc, name=f"million/{k}")


def test_default_gating_takes_the_long_schedule_without_a_vertical_barrier(tape):
    from finmlkit_amd import _ffi, label
    ts, px, lc = tape
    n = len(ts)
    rng = np.random.default_rng(6)
    ev = np.sort(rng.choice(n - 2, 2000, replace=False)).astype(np.int64)
    tg = _sigma(lc, 20000) * (0.5 + 3 * rng.random(len(ev)))
    want, d = check_tb_bits(ts, px, ev, tg, (1.0, 1.0), np.inf, 1.0, None, 0.0, None, lc, name="million/inf")
    assert d["schedule"] == 1 and d["opened"] > 0
    long_paths = int((want[1] - ev > 64 * BLOCK).sum())
    assert long_paths > 100                                             # paths of many blocks ...
    assert d["walked"] < 4 * BLOCK * len(ev)                            # ... of which only the touched ones were walked
    with forced(None):
        label.triple_barrier(ts, px, ev, tg, (1.0, 1.0), 5.0, 1.0, None, 0.0)
    assert diag_last(_ffi.default_context())["schedule"] == 0           # a 5 s barrier: ~100 ticks, the direct walk
    wide = np.full(len(ev), 10.0)                                       # barriers nothing reaches: every path ends at n - 1
    check_tb_bits(ts, px, ev[:300], wide[:300], (1.0, 1.0), np.inf, 1.0, None, 0.0, "long", lc, name="million/inf_wide")
    check_tb_bits(ts, px, ev[:300], wide[:300], (1.0, 1.0), np.inf, 1.0, sd_for(ev[:300]), 0.0, "long", lc,
                  name="million/inf_wide_meta")


def sd_for(ev):
    return (np.asarray(ev) % 3 - 1).astype(np.int8)


@pytest.mark.parametrize("schedule", ["direct", "long"])
def test_edges(tape, schedule):
    ts, px, lc = tape
    n = len(ts)
    # a window with no tick in it: a barrier of 1 ns (every event is skipped unless the next tick has the same timestamp)
    ev = np.arange(0, 5000, 50, dtype=np.int64)
    tg = np.full(len(ev), 1e-3)
    want, d = check_tb_bits(ts, px, ev, tg, (1.0, 1.0), 1e-9, 0.0, None, 0.0, schedule, lc, max_skipped_pct=100.0)
    assert want[4].sum() > 0.9 * len(ev) and np.array_equal(want[1][want[4]], ev[want[4]])
    # a touch exactly at t1_idx: the target is the return at t1 itself, for windows the path stays inside before
    vb = 60.0
    ev = np.arange(1000, 400_000, 199, dtype=np.int64)
    t1 = np.searchsorted(ts.astype(np.float64), ts[ev].astype(np.float64) + vb * 1e9, side="right") - 1
    tg = np.abs(lc[t1] - lc[ev])
    keep = tg > 0
    want, _ = check_tb_bits(ts, px, ev[keep], tg[keep], (1.0, 1.0), vb, 1.0, None, 0.0, schedule, lc, name="edges/touch_at_t1")
    at_t1 = want[1] == t1[keep]
    assert at_t1.sum() >= 5                       # the inputs do exercise the touch_idx == t1_idx branch
    # block table boundaries: event, touch and t1_idx on the first and the last tick of a block
    ev = np.array([BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK, 64 * BLOCK - 1, 64 * BLOCK, 65 * BLOCK - 1, 128 * BLOCK],
                  dtype=np.int64)
    n_t1, n_touch = 0, 0
    # boundary ticks at which the price moves (a first touch needs a new extreme) and after which the clock does (a t1_idx there)
    def boundary(k0, off):
        return next(k * BLOCK + off for k in range(k0, k0 + 60)
                    if px[k * BLOCK + off] != px[k * BLOCK + off - 1] and ts[k * BLOCK + off + 1] > ts[k * BLOCK + off])
    targets = [boundary(3, -1), boundary(3, 0), boundary(130, -1), boundary(130, 0), boundary(192, 0)]
    assert all(t % BLOCK in (0, BLOCK - 1) for t in targets)
    for target_tick in targets:
        # t1_idx on the target tick: the barrier ends between it and the next tick; nothing touches before
        e = ev[ev < target_tick - 1]
        vbs = ((ts[target_tick] - ts[e]) + 0.5 * (ts[target_tick + 1] - ts[target_tick])) / 1e9
        for i, v in zip(e, vbs):
            w, _ = check_tb_bits(ts, px, np.array([i]), np.array([10.0]), (1.0, 1.0), float(v), 0.0, None, 0.0, schedule, lc)
            assert w[1][0] == target_tick and w[3][0] < 1.0
            n_t1 += 1
        # first touch on the target tick: events (block boundaries among them) whose path reaches a new extreme exactly there;
        # the target is that extreme, the other barrier is disabled, no vertical barrier
        here = 0
        cand = np.unique(np.concatenate([e, np.arange(target_tick - 5000, target_tick)]))
        for i in cand[cand >= 0]:
            r = lc[i + 1:target_tick + 1] - lc[i]
            before = r[:-1]
            if r[-1] > 0 and (len(before) == 0 or r[-1] > before.max()):
                hb, tgt = (np.inf, 1.0), r[-1]
            elif r[-1] < 0 and (len(before) == 0 or r[-1] < before.min()):
                hb, tgt = (1.0, np.inf), -r[-1]
            else:
                continue
            if here >= 12 and i not in e:
                continue
            w, _ = check_tb_bits(ts, px, np.array([i]), np.array([tgt]), hb, np.inf, 0.0, None, 0.0, schedule, lc)
            assert w[1][0] == target_tick and w[3][0] == 1.0
            here += 1
        assert here > 0, f"no event touches first at tick {target_tick}"
        n_touch += here
    assert n_t1 >= 30 and n_touch >= 5
    _counts.record(f"labels/edges/{schedule}", events_compared=int(keep.sum()) + n_t1 + n_touch, events_skipped=0,
                   t1_on_block_boundary=n_t1, touch_on_block_boundary=n_touch)


@pytest.mark.parametrize("n", [2, 65, BLOCK - 1, BLOCK, BLOCK + 1])
@pytest.mark.parametrize("schedule", ["direct", "long"])
def test_small_tapes(orc, n, schedule):
    ts, px, _, _ = orc.synth(9, 0, n)
    ev = np.arange(0, n - 1, max(1, n // 40), dtype=np.int64)
    tg = np.full(len(ev), 2e-5)
    check_tb_bits(ts, px, ev, tg, (1.0, 1.0), np.inf, 0.0, None, 0.0, schedule)
    check_tb_bits(ts, px, ev, tg * 1e4, (1.0, 1.0), 3600.0, 0.0, sd_for(ev), 0.0, schedule, max_skipped_pct=100.0)


def test_argument_errors_on_the_device():
    from finmlkit_amd import label
    ts = np.arange(100, dtype=np.int64) * 10 ** 9
    px = np.linspace(100, 101, 100)
    with pytest.raises(ValueError):
        label.triple_barrier(ts, px, np.array([5, 100]), np.array([0.1, 0.1]), (1.0, 1.0), 5.0, 0.0, None, 0.0)
    with pytest.raises(ValueError):
        label.triple_barrier(ts, px, np.array([-1]), np.array([0.1]), (1.0, 1.0), 5.0, 0.0, None, 0.0)
    with pytest.raises(ValueError):
        label.average_uniqueness(ts, np.array([5]), np.array([100]))
    with pytest.raises(ValueError):
        label.average_uniqueness(ts, np.array([5]), np.array([4]))
    with pytest.raises(ValueError):
        label.return_attribution(np.array([5]), np.array([100]), px, np.ones(100, np.int16), False)
    with pytest.raises(ValueError, match="cannot normalize"):
        label.return_attribution(np.array([5]), np.array([9]), np.ones(100), np.ones(100, np.int16), True)


# ---------------------------------------------------------------------------------------------- weights against the helper
def check_weights(ts, px, ev, tch, name):
    from finmlkit_amd import label
    avg, conc = label.average_uniqueness(ts, ev, tch)
    wavg, wconc = H.average_uniqueness(ts, ev, tch)
    assert_bits(conc, wconc, name + "/concurrency")
    rel = np.max(np.abs(avg - wavg) / wavg)
    watt, bound = H.return_attribution(ev, tch, px, wconc, False)
    att = label.return_attribution(ev, tch, px, conc, False)
    print(name, "avg uniqueness max rel", rel, "attribution max err / bound", np.max(np.abs(att - watt) / np.maximum(bound, 1e-300)))
    assert rel <= 1e-9
    assert np.all(np.abs(att - watt) <= bound)
    _counts.record(f"labels/weights/{name}", events_compared=len(ev), events_skipped=0)


def test_weights_vs_helper(tape):
    ts, px, lc = tape
    n = len(ts)
    rng = np.random.default_rng(8)
    ev = rng.choice(n - 2, 4000, replace=False).astype(np.int64)
    length = np.where(rng.random(len(ev)) < 0.2, rng.integers(0, 200_000, len(ev)), rng.integers(0, 3000, len(ev)))
    tch = np.minimum(ev + length, n - 1)
    ev[:6] = [0, 0, BLOCK - 1, BLOCK, 5 * BLOCK, n - 1]
    tch[:6] = [0, n - 1, BLOCK, 2 * BLOCK - 1, 5 * BLOCK, n - 1]
    check_weights(ts, px, ev, tch, "million")


def test_int16_wrap_around():
    from finmlkit_amd import label
    n, m = 5000, 40_000
    ts = np.arange(n, dtype=np.int64)
    ev = np.full(m, 100, np.int64)
    tch = np.full(m, 200, np.int64)
    tch[:10] = 300
    ctx_conc = H.concurrency(n, ev, tch)
    assert ctx_conc[150] == np.int16(m - 65536) and ctx_conc[250] == 10
    from finmlkit_amd import _ffi
    conc = np.empty(n, np.int16)
    _ffi.default_context().call("fmk_label_concurrency", _ffi.ptr(ev), _ffi.ptr(tch), C.c_int64(m), C.c_int64(n), _ffi.ptr(conc))
    assert_bits(conc, ctx_conc, "wrap")
    _counts.record("labels/int16_wrap", events_compared=m, events_skipped=0)


# ---------------------------------------------------------------------------------------------- resident pipeline
def test_resident_pipeline():
    """synth -> CUSUM closes -> ewmst targets -> labels -> weights without a host copy of a tick column on the way."""
    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64
    n = 20_000_000
    t = engine.DeviceTrades.synth(n, seed=11)
    ctx = t.ctx
    r = t.lagged_returns(5.0, True)
    sigma = t.ewmst(r, 60.0)
    d_sig = DeviceArray(ctx, n, np.float64)
    ctx.call("fmk_d2d", d_sig.p, sigma.p, C.c_size_t(n * 8))           # the indexer forward-fills its sigma in place
    m = c_i64()
    d_all = DeviceArray(ctx, n, np.int64)
    ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, d_sig.p, c_i64(n), c_f64(1e-5), c_f64(2.0), d_all.p, c_i64(n),
             C.byref(m), None)
    closes = d_all.view(1, m.value - 1).to_host()
    closes = closes[::max(1, len(closes) // 20000)]
    ts_last = t.first_last_ts()[1]
    ts_ev = t.gather_ts(DeviceArray.from_host(ctx, closes)).to_host()
    ev = closes[ts_ev + 600 * 10 ** 9 <= ts_last]
    assert len(ev) > 1000
    d_ev = DeviceArray.from_host(ctx, ev)
    d_tg = DeviceArray(ctx, len(ev), np.float64)
    ctx.call("fmk_gather_i64_dev", d_sig.p, c_i64(n), d_ev.p, c_i64(len(ev)), d_tg.p)      # 8-byte gather: the bits of sigma
    lab, tch, ret, rat, skipped = t.triple_barrier(d_ev, d_tg, (1.0, 1.0), 600.0, 1.0)
    conc = t.label_concurrency(d_ev, tch)
    avg, att = t.label_weights(d_ev, tch, conc)
    # ---- now download and compare
    ts, px, _, _ = t.to_numpy()
    tg = d_tg.to_host()
    assert np.all(np.isfinite(tg))
    w = H.triple_barrier(ts, px, ev, tg, (1.0, 1.0), 600.0, 1.0, None, 0.0)
    assert skipped.to_host()[0] == w[4].sum() and w[4].sum() * 100 < len(ev)
    for g, x, what in zip((lab, tch, ret, rat), w[:4], ("labels", "touch_idx", "returns", "ratios")):
        assert_bits(g.to_host(), x, "resident/" + what)
    wavg, wconc = H.average_uniqueness(ts, ev, w[1])
    assert_bits(conc.to_host(), wconc, "resident/concurrency")
    assert np.max(np.abs(avg.to_host() - wavg) / wavg) <= 1e-9
    watt, bound = H.return_attribution(ev, w[1], px, wconc, False)
    assert np.all(np.abs(att.to_host() - watt) <= bound)
    _counts.record("labels/resident", events_compared=len(ev), events_skipped=int(w[4].sum()))


# ---------------------------------------------------------------------------------------------- the reference's own test calls
def test_reference_test_calls_through_the_package():
    """Every call the reference's tests/labels make (tests/golden/label_refcalls.*), replayed through finmlkit_amd.label."""
    from finmlkit_amd import label
    from tests import _label_refcalls as L
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # skipped events announce themselves
        c = L.replay(label, only_host=False)
    assert c["calls_replayed"] + c["not_comparable"] == c["calls_total"] and c["calls_left_to_the_gpu"] == 0
    assert c["calls_replayed"] >= 120 and c["calls_raising"] == 11
    _counts.record("labels/refcalls", **c)
