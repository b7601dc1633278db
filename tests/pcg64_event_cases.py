"""Cases that put the device PCG64 decoder (mcmc_gpu_amd/csrc/pcg64_device.h: pcg::Stream) at its rare stream events, and the
finder that makes them.  NumPy and oracle/pcg64_oracle.py only; importable without torch.

Terms.  A draw is one 64-bit output.  A start is a draw that begins a normal.  A window is 64 consecutive draws decoded by one
wavefront; a pass of normals_mw<4> is four windows.  A plane is one call of normals / normals_mw (`count` normals), and its first
pass begins at its first draw.  Every event below is stated by OFFSETS from the first draw of the plane under test, with every
draw before the event on the ziggurat's fast path: then offset o is lane o % 64 of window o // 64 of the first pass, no window
before it is cut, and a start at o is a start whatever the decoder does.  What follows the event is whatever the stream holds.

A case is (name, harness, shape, event, params, state):
    harness  'grid'   gsm_sgs_grid_draw_pcg64, normal draws: shape n = cells listed = cells without a value = normals wanted; the
                      shuffle of the n cells comes first (none for n == 1).  One-wave Stream::normals.
             'draw'   gsm_draw_pcg64, one step: shape (min_x, max_x, min_y, max_y, steps, nugget_max) of RandField.set_block_sizes;
                      params['stream'] names the generator the case is about ('rf', default, or 'ch'), the other one starts at
                      OTHER_STATE; params['plane'] (default 0) the plane under test.  Four-wave Stream::normals_mw<4>.
             'small'  gsm_sgs_draw_pcg64, one iteration on synthetic.sgs_template(SMALL_H, transform=False): shape (H, block_min_x,
                      block_max_x, block_min_y, block_max_y)
    state    ('pos', p)       numpy.random.PCG64(SEED) advanced by p draws, no cached word
             ('seed', s)      numpy.random.default_rng(s)
             ('words', (..))  the six words of GsmEngine.pack_pcg64_states (constructed: XSL-RR inverted, see state_before)
check(case) shows with NumPy alone that the case reaches its event (tests/test_pcg64_events_host.py runs it for every case);
find_all() regenerates CASES (python tests/pcg64_event_cases.py prints the table)."""
import collections
import functools
import math
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import pcg64_oracle as po  # noqa: E402

SEED = 2024
N_SCAN = 5_000_000
SMALL_H = 96
M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1
MULT_INV = pow(po.PCG_MULT, -1, 1 << 128)
KI = np.array(po.KI, dtype=np.uint64)
FAST, WEDGE, TAIL = 0, 1, 2                      # how a draw LOOKS when decoded as a start

Case = collections.namedtuple("Case", "name harness shape event params state")


# ---- generator states ------------------------------------------------------------------------------------------------------------
def pack(st):
    """Six words of a bit_generator.state dict (GsmEngine.pack_pcg64_states without torch)."""
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    return (s & M64, s >> 64, inc & M64, inc >> 64, int(st["has_uint32"]), int(st["uinteger"]))


def state_dict(w):
    return {"bit_generator": "PCG64", "state": {"state": w[0] | (w[1] << 64), "inc": w[2] | (w[3] << 64)}, "has_uint32": w[4],
            "uinteger": w[5]}


def generator(w):
    bg = np.random.PCG64(0)
    bg.state = state_dict(w)
    return np.random.Generator(bg)


def words_at(pos):
    bg = np.random.PCG64(SEED)
    bg.advance(int(pos))                         # negative deltas go backwards
    return pack(bg.state)


def words(case):
    kind, v = case.state
    if kind == "pos":
        return words_at(v)
    if kind == "seed":
        return pack(np.random.default_rng(v).bit_generator.state)
    return tuple(int(x) for x in v)


OTHER_STATE = pack(np.random.default_rng(11).bit_generator.state)


def state_before(out64, hi, inc):
    """The 128-bit LCG state whose NEXT draw is out64, the state behind that draw having the high word `hi`: XSL-RR gives
    rotr64(hi ^ lo, hi >> 58), so lo = rotl64(out64, hi >> 58) ^ hi, and the LCG step is inverted with mult^-1 mod 2^128."""
    rot = hi >> 58
    lo = (((out64 << rot) | (out64 >> ((64 - rot) & 63))) & M64) ^ hi
    return (((hi << 64 | lo) - inc) * MULT_INV) & M128


def rejected_word(n, j):
    """A 32-bit word that Lemire's bounded rejection refuses for the range n: (w * n) mod 2^32 < 2^32 mod n.  The candidates are
    ceil(k * 2^32 / n), the smallest w with (w * n) >> 32 == k; the first k >= j whose candidate is refused is taken."""
    for k in range(j, n):
        w = -((-k << 32) // n)
        if ((w * n) & M32) < (1 << 32) % n:
            return w
    raise ValueError("no rejected word")


def accepted_word(n, v):
    """A word that gives v in [0, n) at once."""
    w = ((v << 32) // n) + 3
    assert ((w * n) & M32) >= (1 << 32) % n and (w * n) >> 32 == v
    return w


def constructed(lo32, hi32, has32=0, cached=0, salt=0):
    """Six words of a generator (increment of PCG64(SEED)) whose next 64-bit draw has the halves lo32, hi32."""
    inc = np.random.PCG64(SEED).state["state"]["inc"]
    s = state_before((hi32 << 32) | lo32, 0x9E3779B97F4A7C15 ^ (salt * 0x100000001B3 & M64), inc)
    return (s & M64, s >> 64, inc & M64, inc >> 64, has32, cached)


# ---- what NumPy does with a stream -----------------------------------------------------------------------------------------------
def looks(raw):
    """FAST / WEDGE / TAIL per raw draw: how random_standard_normal takes it IF it begins a normal."""
    idx = raw & np.uint64(0xFF)
    rabs = (raw >> np.uint64(9)) & np.uint64((1 << 52) - 1)
    slow = rabs >= KI[idx.astype(np.int64)]
    return slow.astype(np.uint8) + (slow & (idx == 0)).astype(np.uint8)


def walk(raw, count):
    """random_standard_normal (numpy/random/src/distributions/distributions.c) `count` times over the raw draws, as
    oracle/pcg64_oracle.Pcg64.standard_normal states it, keeping what it did.  Returns (attempts, draws consumed, values);
    an attempt is (offset of the start, 'fast' | 'wacc' | 'wrej' | 'tail', runs of the tail loop)."""
    att, vals, p = [], [], 0
    dbl = lambda r: (int(r) >> 11) * (1.0 / 9007199254740992.0)
    for _ in range(count):
        while True:
            o, r = p, int(raw[p])
            p += 1
            idx = r & 0xFF
            r >>= 8
            rabs = (r >> 1) & 0x000FFFFFFFFFFFFF
            x = rabs * po.WI[idx]
            if r & 1:
                x = -x
            if rabs < po.KI[idx]:
                att.append((o, "fast", 0)); vals.append(x)
                break
            if idx == 0:
                runs = 0
                while True:
                    runs += 1
                    xx = -po.ZIG_INV_R * math.log1p(-dbl(raw[p]))
                    yy = -math.log1p(-dbl(raw[p + 1]))
                    p += 2
                    if yy + yy > xx * xx:
                        break
                att.append((o, "tail", runs)); vals.append(-(po.ZIG_R + xx) if ((rabs >> 8) & 1) else po.ZIG_R + xx)
                break
            u = dbl(raw[p])
            p += 1
            if (po.FI[idx - 1] - po.FI[idx]) * u + po.FI[idx] < math.exp(-0.5 * x * x):
                att.append((o, "wacc", 0)); vals.append(x)
                break
            att.append((o, "wrej", 0))
    return att, p, vals


def pairs(shape):
    """RandField.get_block_sizes of a 'draw' shape: row 0 widths, row 1 heights."""
    min_x, max_x, min_y, max_y, steps, _ = shape
    w, h = np.meshgrid(np.linspace(min_x, max_x, steps, dtype=int), np.linspace(min_y, max_y, steps, dtype=int))
    return np.array([(w // 2 * 2).flatten(), (h // 2 * 2).flatten()])


@functools.lru_cache(maxsize=None)
def small_template():
    """(chain, is_data) of the 'small' harness."""
    from mcmc_gpu_amd import synthetic
    prob, ch = synthetic.sgs_template(SMALL_H, transform=False)
    return ch, ~np.isnan(prob["cond_bed"])


class _Spy:
    """A Generator as chain_sgs_gpu._draw_iteration uses one, remembering where its standard_normal call began."""

    def __init__(self, g):
        self.g, self.before, self.count = g, None, 0

    def integers(self, **kw):
        return self.g.integers(**kw)

    def shuffle(self, x):
        self.g.shuffle(x)

    def standard_normal(self, n):
        self.before, self.count = pack(self.g.bit_generator.state), int(n)
        return self.g.standard_normal(n)

    def random(self):
        return self.g.random()


def to_plane(case, w=None):
    """NumPy's calls of the harness up to the plane under test: (six words at the plane's first draw, normals wanted)."""
    g = generator(words(case) if w is None else w)
    if case.harness == "grid":
        n = case.shape
        inds = np.stack([np.zeros(n, dtype=np.int64), np.arange(n)], axis=1)
        g.shuffle(inds)                                                      # interpolate._Plan.draws
        return pack(g.bit_generator.state), n
    if case.harness == "draw":
        P = pairs(case.shape)
        i = int(g.integers(low=0, high=P.shape[1], size=1)[0])
        B = int(P[0, i]) * int(P[1, i])
        g.random(); g.random(); g.random()                                   # scale, nugget, range (isotropic)
        for _ in range(case.params.get("plane", 0)):
            g.normal(size=B)
        return pack(g.bit_generator.state), B
    ch, is_data = small_template()
    spy = _Spy(g)
    ch._draw_iteration(spy, is_data)
    return spy.before, spy.count


View = collections.namedtuple("View", "start count att n_draws values look")


def view(case, w=None):
    start, count = to_plane(case, w)
    if start is None:
        return None
    raw = generator(start).bit_generator.random_raw(max(1024, 3 * count + 512))
    att, n_draws, vals = walk(raw, count)
    return View(start, count, att, n_draws, np.array(vals), looks(raw))


def lemire_trace(case):
    """The harness's integer draws of the generator the case is about, through the oracle: per call (value, tokens), a token per
    32-bit word tried -- L the low half of a fresh draw, H the cached high half, lower case when Lemire's test rejects it -- then
    (has_uint32, raw draws consumed) behind the calls of params['pattern']."""
    w = words(case)
    g = po.Pcg64(w[0] | (w[1] << 64), w[2] | (w[3] << 64), w[4], w[5])
    if case.harness == "draw":
        P = pairs(case.shape)
        calls = [(0, P.shape[1])] if case.params.get("stream", "rf") == "rf" else [(0, case.params["H"]), (0, case.params["H"])]
    else:
        H, min_x, max_x, min_y, max_y = case.shape
        calls = [(0, H), (0, H), (min_x, max_x), (min_y, max_y)]
    out = []
    for low, high in calls[:len(case.params["pattern"])]:
        n, tok = high - low, ""
        thr = (1 << 32) % n
        while True:
            src = "H" if g.has_uint32 else "L"
            m = g.next_uint32() * n
            if (m & M32) >= thr:
                tok += src
                break
            tok += src.lower()
        out.append((low + (m >> 32), tok))
    return out, g.has_uint32, g.n_raw, g


# ---- the events: check(case) raises AssertionError unless the case reaches its event ------------------------------------------------
def _at(v, o):
    hit = [a for a in v.att if a[0] == o]
    return hit[0] if hit else None


def _fast(v, a, b):
    assert b >= a and np.all(v.look[a:b] == FAST), f"draws {a} .. {b} of the plane are not all fast"


def _ev_tail(v, p):
    """A tail start in lane `lane` of window `window` of the first pass; runs / min_runs of the tail loop."""
    o = 64 * p.get("window", 0) + p["lane"]
    _fast(v, 0, o)
    a = _at(v, o)
    assert a is not None and a[1] == "tail" and v.look[o] == TAIL, a
    assert a[2] == p["runs"] if "runs" in p else a[2] >= p.get("min_runs", 1), a


def _ev_two_tails(v, p):
    """Two tail starts in the first window: the decode sees both, the cut is before the first."""
    o, o2 = p["lane"], p["lane2"]
    _fast(v, 0, o)
    a, b = _at(v, o), _at(v, o2)
    assert o < o2 < 64 and a and b and a[1] == b[1] == "tail" and v.look[o2] == TAIL and o2 > o + 2 * a[2]


def _ev_wedge63(v, p):
    """A wedge start in lane 63 of window `window`: its uniform is the next window's first draw."""
    o = 64 * p.get("window", 0) + 63
    _fast(v, 0, o)
    a = _at(v, o)
    assert a is not None and a[1] == ("wacc" if p["accepted"] else "wrej")


def _ev_wedge_wedge(v, p):
    """A wedge start whose uniform looks like a wedge start itself (it is none), then a real wedge start."""
    o = p["lane"]
    _fast(v, 0, o)
    a, b = _at(v, o), _at(v, o + 2)
    assert a and b and a[1][0] == "w" and b[1][0] == "w" and v.look[o + 1] == WEDGE and _at(v, o + 1) is None and o + 3 < 64


def _ev_wedge_taillook(v, p):
    """A wedge start whose uniform looks like a tail start: no start there, so the window is not cut there -- every other draw of
    the window is fast and all 64 are consumed in one pass."""
    o = p["lane"]
    _fast(v, 0, o)
    _fast(v, o + 2, 64)
    a = _at(v, o)
    assert a and a[1][0] == "w" and v.look[o + 1] == TAIL and _at(v, o + 1) is None and o + 1 < 64 and v.n_draws > 64


def _ev_end_fast(v, p):
    """The last normal is a fast draw at offset `last` (lane 63 of a window, or the 256th draw of a pass); with wedge=True an
    accepted wedge start lies before it, so the window is not the all-fast one."""
    last = p["last"]
    assert v.att[-1] == (last, "fast", 0) and v.n_draws == last + 1
    kinds = [a[1] for a in v.att]
    if p.get("wedge"):
        assert kinds.count("wacc") == 1 and set(kinds) == {"fast", "wacc"} and v.count == last
    else:
        assert set(kinds) == {"fast"} and v.count == last + 1


def _ev_end_wacc(v, p):
    """The last normal is an accepted wedge start in lane `lane`: its uniform is consumed and nothing behind it."""
    o = p["lane"]
    _fast(v, 0, o)
    assert v.att[-1] == (o, "wacc", 0) and v.n_draws == o + 2 and v.count == o + 1


def _ev_after(v, p):
    """The draw behind the last normal would start a wedge / a tail: NumPy never makes it."""
    _fast(v, 0, v.count)
    assert v.n_draws == v.count < 64 and v.look[v.count] == (WEDGE if p["what"] == "wedge" else TAIL)


def _ev_rej_before_last(v, p):
    """A rejected wedge start directly before the last normal."""
    o = p["lane"]
    _fast(v, 0, o)
    assert v.att[-2:] == [(o, "wrej", 0), (o + 2, "fast", 0)] and v.n_draws == o + 3 and o + 2 < 63


def _ev_end_tail(v, p):
    """The last normal is a tail draw."""
    o = p["lane"]
    _fast(v, 0, o)
    assert v.att[-1][:2] == (o, "tail") and v.count == o + 1


def _ev_end_inside(v, p):
    """Four-wave: the plane ends inside window `window` of the first pass, every normal fast, while a later draw of the pass (offset
    `later`, in a later window where there is one) looks like a tail or wedge start."""
    w, e = p["window"], p["later"]
    _fast(v, 0, v.count)
    assert 64 * w < v.count <= 64 * (w + 1) and v.n_draws == v.count
    assert (e >= 64 * (w + 1) if w < 3 else e > v.count) and e < 256 and v.look[e] != FAST


def _ev_cut_before_end(v, p):
    """Four-wave: a tail start cuts window `window`; had every draw been fast, the plane would have ended in a later window."""
    o = 64 * p["window"] + p["lane"]
    _fast(v, 0, o)
    a = _at(v, o)
    assert a and a[1] == "tail" and 64 * (p["window"] + 1) < v.count <= 256 and p["lane"] > 0


def _ev_all_fast(v, p):
    """`count` fast draws."""
    _fast(v, 0, v.count)
    assert v.n_draws == v.count == p["count"]


def _ev_lemire(case):
    """Lemire rejections where params['pattern'] says, has_uint32 and the raw draws consumed behind them; NumPy agrees."""
    tr, has32, n_raw, orc = lemire_trace(case)
    p = case.params
    assert tuple(t for _, t in tr) == tuple(p["pattern"]), tr
    assert has32 == p["has32"] and n_raw == p["n_raw"]
    if "low" in p:
        assert case.shape[1 + 2 * p["low"][0]] == p["low"][1] > 0             # the rejected call has low > 0
    g = generator(words(case))
    if case.harness == "draw":
        calls = [(0, pairs(case.shape).shape[1])] if p.get("stream", "rf") == "rf" else [(0, p["H"]), (0, p["H"])]
    else:
        H, a, b, c, d = case.shape
        calls = [(0, H), (0, H), (a, b), (c, d)]
    for (low, high), (val, _) in zip(calls, tr):
        assert int(g.integers(low=low, high=high, size=1)[0]) == val
    assert g.bit_generator.state == orc.numpy_state()


EVENTS = dict(tail=_ev_tail, two_tails=_ev_two_tails, wedge63=_ev_wedge63, wedge_wedge=_ev_wedge_wedge,
              wedge_taillook=_ev_wedge_taillook, end_fast=_ev_end_fast, end_wacc=_ev_end_wacc, after=_ev_after,
              rej_before_last=_ev_rej_before_last, end_tail=_ev_end_tail, end_inside=_ev_end_inside,
              cut_before_end=_ev_cut_before_end, all_fast=_ev_all_fast)


def check(case, v=None):
    if case.event == "lemire":
        return _ev_lemire(case)
    v = view(case) if v is None else v
    assert v is not None and v.count == len([a for a in v.att if a[1] != "wrej"])
    if case.harness == "draw":
        P = pairs(case.shape)
        assert P.shape[1] == 1 and v.count == int(P[0, 0]) * int(P[1, 0])
    EVENTS[case.event](v, case.params)


def reaches(case, v=None):
    try:
        check(case, v)
        return True
    except (AssertionError, IndexError):
        return False


# ---- the finder ----------------------------------------------------------------------------------------------------------------
class Scan:
    """N_SCAN raw draws of PCG64(SEED), classified; run[i] = fast draws directly before draw i."""

    def __init__(self):
        self.look = looks(np.random.PCG64(SEED).random_raw(N_SCAN))
        last_slow = np.maximum.accumulate(np.where(self.look != FAST, np.arange(N_SCAN), -1))
        self.run = np.zeros(N_SCAN, dtype=np.int64)
        self.run[1:] = np.arange(1, N_SCAN) - 1 - last_slow[:-1]

    def where(self, o, *kinds):
        """Plane starts p such that draws p .. p + o - 1 are fast and draws p + o, p + o + 1, .. look like `kinds` (None: any)."""
        n = N_SCAN - 600
        ok = self.run[:n] >= o
        for k, kind in enumerate(kinds):
            if kind is not None:
                ok &= self.look[k:n + k] == kind
        q = np.flatnonzero(ok) - o
        return q[q > 4096]


def _int_state(w):
    return w[0] | (w[1] << 64)


def land(case, pos):
    """('pos', p): a state of PCG64(SEED) from which the harness's calls before the plane under test end exactly on draw `pos`
    of the stream -- the prefix is backed off by d draws, d near its expected length, and replayed with NumPy."""
    target = _int_state(words_at(pos))
    if case.harness == "grid":
        n = case.shape
        if n == 1:
            return ("pos", int(pos))
        mean = 0.5 * sum((1 << i.bit_length()) / (i + 1) for i in range(1, n))
        ds = sorted(range(max((n - 1) // 2, int(mean) - 16), int(mean) + 17), key=lambda d: abs(d - mean))
    else:
        B, pl = int(np.prod(pairs(case.shape)[:, 0])), case.params.get("plane", 0)
        ds = [3 + pl * B + k for k in range(0, 1 if pl == 0 else 10 * pl)]
    for d in ds:
        w = words_at(pos - d)
        if _int_state(to_plane(case, w)[0]) == target:
            return ("pos", int(pos - d))
    return None


D1 = lambda bw, bh, nug=0.0: (bw, bw, bh, bh, 1, nug)          # a 'draw' shape with the single block bw x bh


def specs(sc):
    """(name, harness, shape, event, params, plane starts to try).  Offsets are chosen so that a four-wave plane length is a
    product of two even numbers."""
    W = sc.where
    out = []
    add = lambda *a: out.append(a)
    # ---- one-wave: Stream::normals through the whole-grid draw kernel ---------------------------------------------------------
    add("g-tail-head-1", "grid", 96, "tail", dict(lane=0, runs=1), W(0, TAIL))
    add("g-tail-head-2", "grid", 96, "tail", dict(lane=0, runs=2), W(0, TAIL))
    add("g-tail-head-3", "grid", 96, "tail", dict(lane=0, min_runs=3), W(0, TAIL))
    for lane in (1, 31, 63):
        add(f"g-tail-lane{lane}", "grid", 96, "tail", dict(lane=lane), W(lane, TAIL))
    add("g-two-tails", "grid", 96, "two_tails", None, None)
    add("g-wedge63-acc", "grid", 65, "wedge63", dict(accepted=True), W(63, WEDGE))
    add("g-wedge63-rej", "grid", 65, "wedge63", dict(accepted=False), W(63, WEDGE))
    add("g-wedge-wedge", "grid", 96, "wedge_wedge", dict(lane=9), W(9, WEDGE, WEDGE, WEDGE))
    add("g-wedge-taillook", "grid", 96, "wedge_taillook", dict(lane=20), W(20, WEDGE, TAIL))
    add("g-end-fast63-all-fast", "grid", 64, "end_fast", dict(last=63), W(64))
    add("g-end-fast63-after-wedge", "grid", 63, "end_fast", dict(last=63, wedge=True), W(30, WEDGE))
    add("g-end-wacc-lane40", "grid", 41, "end_wacc", dict(lane=40), W(40, WEDGE))
    add("g-end-wacc-lane63", "grid", 64, "end_wacc", dict(lane=63), W(63, WEDGE))
    add("g-after-wedge", "grid", 33, "after", dict(what="wedge"), W(33, WEDGE))
    add("g-after-tail", "grid", 33, "after", dict(what="tail"), W(33, TAIL))
    add("g-rej-before-last", "grid", 25, "rej_before_last", dict(lane=24), W(24, WEDGE))
    add("g-end-tail", "grid", 18, "end_tail", dict(lane=17), W(17, TAIL))
    add("g-count1-tail", "grid", 1, "end_tail", dict(lane=0), W(0, TAIL))
    add("g-count1-wacc", "grid", 1, "end_wacc", dict(lane=0), W(0, WEDGE))
    add("g-count65-all-fast", "grid", 65, "all_fast", dict(count=65), W(65))
    # ---- four-wave: Stream::normals_mw<4> through the chain draw kernel, one 16 x 16 block unless the plane's end is the event ------
    big = D1(16, 16)
    add("d-tail-head-1", "draw", big, "tail", dict(lane=0, runs=1), W(0, TAIL))
    add("d-tail-head-2", "draw", big, "tail", dict(lane=0, runs=2), W(0, TAIL))
    add("d-tail-head-3", "draw", big, "tail", dict(lane=0, min_runs=3), W(0, TAIL))
    for w, lane in ((0, 1), (0, 31), (0, 63), (1, 0), (2, 0), (3, 0), (1, 17), (3, 40)):
        add(f"d-tail-w{w}-lane{lane}", "draw", big, "tail", dict(window=w, lane=lane), W(64 * w + lane, TAIL))
    add("d-two-tails", "draw", big, "two_tails", None, None)
    for w in (0, 1, 3):
        add(f"d-wedge63-w{w}-acc", "draw", big, "wedge63", dict(window=w, accepted=True), W(64 * w + 63, WEDGE))
    add("d-wedge63-w0-rej", "draw", big, "wedge63", dict(window=0, accepted=False), W(63, WEDGE))
    add("d-wedge63-w3-rej", "draw", big, "wedge63", dict(window=3, accepted=False), W(255, WEDGE))
    add("d-wedge-wedge", "draw", big, "wedge_wedge", dict(lane=9), W(9, WEDGE, WEDGE, WEDGE))
    add("d-wedge-taillook", "draw", big, "wedge_taillook", dict(lane=20), W(20, WEDGE, TAIL))
    add("d-end-256th", "draw", big, "end_fast", dict(last=255), W(256))
    add("d-end-fast63", "draw", D1(8, 8), "end_fast", dict(last=63), W(64))
    add("d-end-wacc-lane31", "draw", D1(4, 8), "end_wacc", dict(lane=31), W(31, WEDGE))
    add("d-end-wacc-lane63", "draw", D1(8, 8), "end_wacc", dict(lane=63), W(63, WEDGE))
    add("d-after-wedge", "draw", D1(4, 8), "after", dict(what="wedge"), W(32, WEDGE))
    add("d-after-tail", "draw", D1(4, 8), "after", dict(what="tail"), W(32, TAIL))
    add("d-rej-before-last", "draw", D1(4, 8), "rej_before_last", dict(lane=31), W(31, WEDGE))
    add("d-end-tail", "draw", D1(4, 8), "end_tail", dict(lane=31), W(31, TAIL))
    for w, shp, later, kind in ((0, D1(4, 8), 100, TAIL), (1, D1(8, 12), 140, WEDGE), (2, D1(10, 16), 200, TAIL),
                                (3, D1(14, 16), 240, WEDGE)):
        B = shp[0] * shp[2]
        add(f"d-end-inside-w{w}", "draw", shp, "end_inside", dict(window=w, later=later), W(B, *([None] * (later - B) + [kind])))
    add("d-cut-w1-before-end-in-w2", "draw", D1(10, 16), "cut_before_end", dict(window=1, lane=22), W(64 + 22, TAIL))
    # ---- plane seams of pcg64_draw_kernel: the event in the first window of plane 1 and of plane 2 -------------------------------
    add("d-seam-plane1-tail", "draw", D1(8, 8), "tail", dict(plane=1, lane=5), W(5, TAIL))
    add("d-seam-plane2-wedge-wedge-unstored", "draw", D1(8, 8), "wedge_wedge", dict(plane=2, lane=9), W(9, WEDGE, WEDGE, WEDGE))
    add("d-seam-plane2-tail-unstored", "draw", D1(8, 8), "tail", dict(plane=2, lane=12), W(12, TAIL))
    add("d-seam-plane1-tail-nugget", "draw", D1(8, 8, 4.0), "tail", dict(plane=1, lane=7), W(7, TAIL))
    add("d-seam-plane2-tail-nugget", "draw", D1(8, 8, 4.0), "tail", dict(plane=2, lane=12), W(12, TAIL))
    add("d-seam-plane2-end-wacc-nugget", "draw", D1(8, 8, 4.0), "end_wacc", dict(plane=2, lane=63), W(63, WEDGE))
    return out


def _two_tails(sc, harness, shape):
    t = np.flatnonzero(sc.look == TAIL)
    t = t[t > 4096]
    for a, b in zip(t[:-1], t[1:]):
        gap = int(b - a)
        o = min(int(sc.run[a]), 62 - gap)
        if gap < 50 and o >= 1:
            yield dict(lane=o, lane2=o + gap), int(a) - o


def find_events(sc):
    out = []
    for name, harness, shape, event, params, starts in specs(sc):
        tries = _two_tails(sc, harness, shape) if event == "two_tails" else ((params, int(p)) for p in starts)
        for prm, pos in tries:
            c = Case(name, harness, shape, event, prm, None)
            # the plane itself first (cheap), then a state from which the harness's prefix ends on it
            w0 = words_at(pos)
            count = shape if harness == "grid" else int(np.prod(pairs(shape)[:, 0]))
            raw = generator(w0).bit_generator.random_raw(1536)
            att, n_draws, vals = walk(raw, count)
            if not reaches(c, View(w0, count, att, n_draws, np.array(vals), looks(raw))):
                continue
            st = land(c, pos)
            if st is None:
                continue
            c = c._replace(state=st)
            check(c)
            out.append(c)
            break
        else:
            raise RuntimeError(f"no case found for {name}")
    return out


H_LEM = 96                                       # 2^32 mod 96 = 64: rejected words exist, and 96 is no power of two


def lemire_cases(small_shape):
    """Constructed states: one 64-bit draw with both halves chosen (and the cached word where the case starts with one)."""
    R, A = rejected_word, accepted_word
    ch = dict(stream="ch", H=H_LEM)
    t25 = (8, 16, 8, 16, 5, 0.0)                 # 25 block sizes: 2^32 mod 25 = 21
    H, min_x, max_x, min_y, max_y = small_shape
    rx = max_x - min_x
    assert (1 << 32) % H > 0 and (1 << 32) % rx > 0 and (1 << 32) % 25 == 21 and min_x > 0
    mk = lambda name, harness, shape, prm, w: Case(name, harness, shape, "lemire", prm, ("words", w))
    return [
        mk("c-low-rejected-cached-serves", "draw", D1(8, 8), dict(ch, pattern=("lH", "L"), has32=1, n_raw=2),
           constructed(R(H_LEM, 37), A(H_LEM, 40), salt=1)),
        mk("c-cached-high-rejected", "draw", D1(8, 8), dict(ch, pattern=("L", "hL"), has32=1, n_raw=2),
           constructed(A(H_LEM, 17), R(H_LEM, 59), salt=2)),
        mk("c-both-halves-rejected", "draw", D1(8, 8), dict(ch, pattern=("lhL", "H"), has32=0, n_raw=2),
           constructed(R(H_LEM, 5), R(H_LEM, 91), salt=3)),
        mk("r-bounded25-low-rejected", "draw", t25, dict(pattern=("lH",), has32=0, n_raw=1), constructed(R(25, 7), A(25, 12), salt=4)),
        mk("r-bounded25-cached-rejected", "draw", t25, dict(pattern=("hL",), has32=1, n_raw=1),
           constructed(A(25, 3), A(25, 4), has32=1, cached=R(25, 19), salt=5)),
        mk("s-integers-0-H-low-rejected", "small", small_shape, dict(pattern=("lH", "L"), has32=1, n_raw=2),
           constructed(R(H, 41), A(H, 40), salt=6)),
        mk("s-integers-block-cached-rejected", "small", small_shape, dict(pattern=("H", "L", "hL"), has32=1, n_raw=2, low=(0, min_x)),
           constructed(A(H, 50), R(rx, 0), has32=1, cached=A(H, 40), salt=7)),
    ]


def small_cases(small_shape):
    """Seeds tried through chain_sgs_gpu._draw_iteration until its normals call holds the event in its first window."""
    want = [("s-tail-in-window", "tail", lambda v: next((dict(lane=a[0]) for a in v.att if a[1] == "tail" and 0 < a[0] < 64), None)),
            ("s-end-on-accepted-wedge", "end_wacc", lambda v: dict(lane=v.att[-1][0]) if v.att[-1][1] == "wacc" and v.att[-1][0] < 63 else None)]
    out = {}
    for seed in range(20000):
        c = Case("", "small", small_shape, "", {}, ("seed", seed))
        v = view(c)
        if v is None or v.count == 0:
            continue
        for name, event, prm in want:
            if name not in out and prm(v) is not None:
                cand = c._replace(name=name, event=event, params=prm(v))
                if reaches(cand, v):
                    out[name] = cand
        if len(out) == len(want):
            return [out[n] for n, _, _ in want]
    raise RuntimeError("no small-scale case found")


def small_shape():
    ch, _ = small_template()
    return (SMALL_H, int(ch.block_min_x), int(ch.block_max_x), int(ch.block_min_y), int(ch.block_max_y))


def find_all():
    shp = small_shape()
    return find_events(Scan()) + lemire_cases(shp) + small_cases(shp)


def _literal(c):
    st = c.state if c.state[0] != "words" else ("words", "(" + ", ".join(hex(x) for x in c.state[1]) + ")")
    st = f"({st[0]!r}, {st[1]})"
    return f"    ({c.name!r}, {c.harness!r}, {c.shape!r}, {c.event!r}, {c.params!r}, {st}),"


# what find_all() returns (1.3 s on one CPU core; every case lies in the first 4 * 10^6 draws of the stream); tests/test_pcg64_events_host.py regenerates and compares
_BIG, _B64, _B32, _T25, _SM = (16, 16, 16, 16, 1, 0.0), (8, 8, 8, 8, 1, 0.0), (4, 4, 8, 8, 1, 0.0), (8, 16, 8, 16, 5, 0.0), (96, 5, 20, 5, 20)
_B64N = (8, 8, 8, 8, 1, 4.0)
_INC = (0xdf440b34fffb7769, 0xc67e5ec6f768fa51)
CASES = [Case(*t) for t in [
    ('g-tail-head-1', 'grid', 96, 'tail', {'lane': 0, 'runs': 1}, ('pos', 4313)),
    ('g-tail-head-2', 'grid', 96, 'tail', {'lane': 0, 'runs': 2}, ('pos', 571922)),
    ('g-tail-head-3', 'grid', 96, 'tail', {'lane': 0, 'min_runs': 3}, ('pos', 3030319)),
    ('g-tail-lane1', 'grid', 96, 'tail', {'lane': 1}, ('pos', 19385)),
    ('g-tail-lane31', 'grid', 96, 'tail', {'lane': 31}, ('pos', 17603)),
    ('g-tail-lane63', 'grid', 96, 'tail', {'lane': 63}, ('pos', 19321)),
    ('g-two-tails', 'grid', 96, 'two_tails', {'lane': 1, 'lane2': 18}, ('pos', 2236844)),
    ('g-wedge63-acc', 'grid', 65, 'wedge63', {'accepted': True}, ('pos', 4134)),
    ('g-wedge63-rej', 'grid', 65, 'wedge63', {'accepted': False}, ('pos', 4417)),
    ('g-wedge-wedge', 'grid', 96, 'wedge_wedge', {'lane': 9}, ('pos', 1370035)),
    ('g-wedge-taillook', 'grid', 96, 'wedge_taillook', {'lane': 20}, ('pos', 3917144)),
    ('g-end-fast63-all-fast', 'grid', 64, 'end_fast', {'last': 63}, ('pos', 4056)),
    ('g-end-fast63-after-wedge', 'grid', 63, 'end_fast', {'last': 63, 'wedge': True}, ('pos', 4375)),
    ('g-end-wacc-lane40', 'grid', 41, 'end_wacc', {'lane': 40}, ('pos', 4380)),
    ('g-end-wacc-lane63', 'grid', 64, 'end_wacc', {'lane': 63}, ('pos', 4135)),
    ('g-after-wedge', 'grid', 33, 'after', {'what': 'wedge'}, ('pos', 4393)),
    ('g-after-tail', 'grid', 33, 'after', {'what': 'tail'}, ('pos', 19395)),
    ('g-rej-before-last', 'grid', 25, 'rej_before_last', {'lane': 24}, ('pos', 4485)),
    ('g-end-tail', 'grid', 18, 'end_tail', {'lane': 17}, ('pos', 4351)),
    ('g-count1-tail', 'grid', 1, 'end_tail', {'lane': 0}, ('pos', 4381)),
    ('g-count1-wacc', 'grid', 1, 'end_wacc', {'lane': 0}, ('pos', 4240)),
    ('g-count65-all-fast', 'grid', 65, 'all_fast', {'count': 65}, ('pos', 4056)),
    ('d-tail-head-1', 'draw', _BIG, 'tail', {'lane': 0, 'runs': 1}, ('pos', 4378)),
    ('d-tail-head-2', 'draw', _BIG, 'tail', {'lane': 0, 'runs': 2}, ('pos', 97413)),
    ('d-tail-head-3', 'draw', _BIG, 'tail', {'lane': 0, 'min_runs': 3}, ('pos', 758778)),
    ('d-tail-w0-lane1', 'draw', _BIG, 'tail', {'window': 0, 'lane': 1}, ('pos', 4377)),
    ('d-tail-w0-lane31', 'draw', _BIG, 'tail', {'window': 0, 'lane': 31}, ('pos', 4347)),
    ('d-tail-w0-lane63', 'draw', _BIG, 'tail', {'window': 0, 'lane': 63}, ('pos', 19385)),
    ('d-tail-w1-lane0', 'draw', _BIG, 'tail', {'window': 1, 'lane': 0}, ('pos', 19384)),
    ('d-tail-w2-lane0', 'draw', _BIG, 'tail', {'window': 2, 'lane': 0}, ('pos', 28374)),
    ('d-tail-w3-lane0', 'draw', _BIG, 'tail', {'window': 3, 'lane': 0}, ('pos', 66178)),
    ('d-tail-w1-lane17', 'draw', _BIG, 'tail', {'window': 1, 'lane': 17}, ('pos', 19367)),
    ('d-tail-w3-lane40', 'draw', _BIG, 'tail', {'window': 3, 'lane': 40}, ('pos', 109219)),
    ('d-two-tails', 'draw', _BIG, 'two_tails', {'lane': 17, 'lane2': 26}, ('pos', 552140)),
    ('d-wedge63-w0-acc', 'draw', _BIG, 'wedge63', {'window': 0, 'accepted': True}, ('pos', 4174)),
    ('d-wedge63-w1-acc', 'draw', _BIG, 'wedge63', {'window': 1, 'accepted': True}, ('pos', 4110)),
    ('d-wedge63-w3-acc', 'draw', _BIG, 'wedge63', {'window': 3, 'accepted': True}, ('pos', 5866)),
    ('d-wedge63-w0-rej', 'draw', _BIG, 'wedge63', {'window': 0, 'accepted': False}, ('pos', 4255)),
    ('d-wedge63-w3-rej', 'draw', _BIG, 'wedge63', {'window': 3, 'accepted': False}, ('pos', 6328)),
    ('d-wedge-wedge', 'draw', _BIG, 'wedge_wedge', {'lane': 9}, ('pos', 1294159)),
    ('d-wedge-taillook', 'draw', _BIG, 'wedge_taillook', {'lane': 20}, ('pos', 1720278)),
    ('d-end-256th', 'draw', _BIG, 'end_fast', {'last': 255}, ('pos', 5790)),
    ('d-end-fast63', 'draw', _B64, 'end_fast', {'last': 63}, ('pos', 4094)),
    ('d-end-wacc-lane31', 'draw', _B32, 'end_wacc', {'lane': 31}, ('pos', 4206)),
    ('d-end-wacc-lane63', 'draw', _B64, 'end_wacc', {'lane': 63}, ('pos', 4174)),
    ('d-after-wedge', 'draw', _B32, 'after', {'what': 'wedge'}, ('pos', 4205)),
    ('d-after-tail', 'draw', _B32, 'after', {'what': 'tail'}, ('pos', 4346)),
    ('d-rej-before-last', 'draw', _B32, 'rej_before_last', {'lane': 31}, ('pos', 4287)),
    ('d-end-tail', 'draw', _B32, 'end_tail', {'lane': 31}, ('pos', 4347)),
    ('d-end-inside-w0', 'draw', _B32, 'end_inside', {'window': 0, 'later': 100}, ('pos', 4278)),
    ('d-end-inside-w1', 'draw', (8, 8, 12, 12, 1, 0.0), 'end_inside', {'window': 1, 'later': 140}, ('pos', 4097)),
    ('d-end-inside-w2', 'draw', (10, 10, 16, 16, 1, 0.0), 'end_inside', {'window': 2, 'later': 200}, ('pos', 66170)),
    ('d-end-inside-w3', 'draw', (14, 14, 16, 16, 1, 0.0), 'end_inside', {'window': 3, 'later': 240}, ('pos', 5881)),
    ('d-cut-w1-before-end-in-w2', 'draw', (10, 10, 16, 16, 1, 0.0), 'cut_before_end', {'window': 1, 'lane': 22}, ('pos', 20219)),
    ('d-seam-plane1-tail', 'draw', _B64, 'tail', {'plane': 1, 'lane': 5}, ('pos', 4307)),
    ('d-seam-plane2-wedge-wedge-unstored', 'draw', _B64, 'wedge_wedge', {'plane': 2, 'lane': 9}, ('pos', 1294028)),
    ('d-seam-plane2-tail-unstored', 'draw', _B64, 'tail', {'plane': 2, 'lane': 12}, ('pos', 4235)),
    ('d-seam-plane1-tail-nugget', 'draw', _B64N, 'tail', {'plane': 1, 'lane': 7}, ('pos', 4305)),
    ('d-seam-plane2-tail-nugget', 'draw', _B64N, 'tail', {'plane': 2, 'lane': 12}, ('pos', 4235)),
    ('d-seam-plane2-end-wacc-nugget', 'draw', _B64N, 'end_wacc', {'plane': 2, 'lane': 63}, ('pos', 4046)),
    ('c-low-rejected-cached-serves', 'draw', _B64, 'lemire', {'stream': 'ch', 'H': 96, 'pattern': ('lH', 'L'), 'has32': 1, 'n_raw': 2},
     ('words', (0x18889193526ded6, 0x9f8d81fc66c38cee) + _INC + (0x0, 0x0))),
    ('c-cached-high-rejected', 'draw', _B64, 'lemire', {'stream': 'ch', 'H': 96, 'pattern': ('L', 'hL'), 'has32': 1, 'n_raw': 2},
     ('words', (0x33a5f8aee22cb5cc, 0xe640f179197e5d3b) + _INC + (0x0, 0x0))),
    ('c-both-halves-rejected', 'draw', _B64, 'lemire', {'stream': 'ch', 'H': 96, 'pattern': ('lhL', 'H'), 'has32': 0, 'n_raw': 2},
     ('words', (0xf57e68ceeff2e3df, 0xf9c9b2e929347a17) + _INC + (0x0, 0x0))),
    ('r-bounded25-low-rejected', 'draw', _T25, 'lemire', {'pattern': ('lH',), 'has32': 0, 'n_raw': 1},
     ('words', (0xc67c11c8cd6b245d, 0x2ec9b962aac9ae02) + _INC + (0x0, 0x0))),
    ('r-bounded25-cached-rejected', 'draw', _T25, 'lemire', {'pattern': ('hL',), 'has32': 1, 'n_raw': 1},
     ('words', (0xb6246b18891d5bcc, 0x1c010df949fb7592) + _INC + (0x1, 0xc28f5c29))),
    ('s-integers-0-H-low-rejected', 'small', _SM, 'lemire', {'pattern': ('lH', 'L'), 'has32': 1, 'n_raw': 2},
     ('words', (0x21180275b6887abe, 0xa5e18c3aa1ba3f5f) + _INC + (0x0, 0x0))),
    ('s-integers-block-cached-rejected', 'small', _SM, 'lemire', {'pattern': ('H', 'L', 'hL'), 'has32': 1, 'n_raw': 2, 'low': (0, 5)},
     ('words', (0x52ecb6c58b123435, 0x2e14087bb3d8f310) + _INC + (0x1, 0x6aaaaaad))),
    ('s-tail-in-window', 'small', _SM, 'tail', {'lane': 39}, ('seed', 23)),
    ('s-end-on-accepted-wedge', 'small', _SM, 'end_wacc', {'lane': 62}, ('seed', 166)),
]]
BY_NAME = {c.name: c for c in CASES}

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    t0 = time.time()
    for c in find_all():
        print(_literal(c))
    print(f"# found in {time.time() - t0:.1f} s", file=sys.stderr)
