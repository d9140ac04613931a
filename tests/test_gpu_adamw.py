"""The AdamW kernels against an independent float64 statement of the update (``oracle.adamw_step_f64``), one step at a time, element
by element: the flat update (``moss_adamw_flat_ex``: segments, periodic rates, shards, extra gradient buffers, the degree-aware SH form,
the device-side step counter and learning-rate table, the guard) and the multi-tensor one (``moss_adamw_multi``).  The update inside the
per-Gaussian backward shares ``adamw.h`` with the flat kernel and is held bit-identical to it by
``test_gpu_ops.py::test_backward_kernel_takes_the_adamw_step``: it is covered through these tests and not repeated here.

Every step is checked from the kernel's OWN float32 state before that step (parameters, gradients, moments, rates as the kernel was
given them), evaluated in float64 -- so the bars do not drift over long runs.

Bars (u = 2^-24, the unit roundoff of float32; V_ABS = 2^-126, the smallest normal float32; all per element, none scaled by max |p|).
The kernel evaluates, every operation rounded once (adamw.h: adamw_element; betas, 1 - beta, bias corrections rounded to float32):
    p1 = p0 (1 - lr wd);  m = b1 m0 + (1-b1) g;  v = b2 v0 + ((1-b2) g) g;  d = sqrt(v) / sqrt(bc2) + eps;  p = p1 - lr/bc1 m / d
with a hardware square root and reciprocal (about 1 ulp each).
  m:  |m - m*| <= 4u (|b1 m0| + |(1-b1) g|).  Two roundings plus the representation error of b1 and 1-b1, each <= u/2 relative to the
      term it multiplies.  Bounding by the magnitudes of the TERMS (not of m) keeps cancellation from causing false failures.
  v:  |v - v*| <= 4u (|b2 v0| + |(1-b2) g^2|) + V_ABS.  Three roundings and the representation errors; V_ABS covers a g^2 that underflows
      (a gradient of 1e-30) or a subnormal flushed to zero.
  p:  |p - p*| <= 4u |p0 lr wd| + U (8u + r) + 1.5 ulp(max(|p0|, |p*|)), where U = lr/bc1 M / d*, M = |b1 m0| + |(1-b1) g| (the term bound
      of m again), d* the float64 denominator and r = (4u d* + sqrt(V_ABS)/sqrt(bc2)) / d* its relative error.  8u: bc1, 1/bc1, lr/bc1,
      the reciprocal (~1 ulp), m r and the error of m itself; r: bc2, its square root and reciprocal, the hardware square root (~1 ulp),
      the relative error of v (halved by the square root), the fma with eps, and an underflowed v.  The ulp term: 1 - lr wd rounds to
      float32 (an absolute error of up to u/2, times p0: < 1/2 ulp of p0), the product and the final fma each round once (1/2 ulp
      each); errors of just over one ulp are seen.
  NaN and +-inf must be exactly where the float64 reference has them.  Elements that the degree-aware form leaves alone must keep their
  moments bit for bit.
The largest error seen for each bar, as a fraction of the bar, is printed at the end of the module (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
V_ABS = 2.0 ** -126
_WORST = {"m": 0.0, "v": 0.0, "p": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nlargest error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))


def _bars(p0, g, m0, v0, lr, beta1, beta2, eps, wd, step, ref):
    """Element-wise bars for (p, m, v) -- module docstring.  Inputs float32 arrays (g: the step's gradient), ``ref`` the float64
    result of the same step."""
    p0, g, m0, v0 = (np.asarray(a, np.float64) for a in (p0, g, m0, v0))
    lr = np.asarray(lr, np.float64) * np.ones_like(p0)
    b1, b2 = float(beta1), float(beta2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        M = np.abs(b1 * m0) + np.abs((1.0 - b1) * g)
        bar_m = 4 * U * M
        bar_v = 4 * U * (np.abs(b2 * v0) + np.abs((1.0 - b2) * g * g)) + V_ABS
        d = np.sqrt(np.maximum(ref[2], 0.0)) / math.sqrt(bc2) + float(eps)
        Uu = lr / bc1 * M / d
        r = (4 * U * d + math.sqrt(V_ABS) / math.sqrt(bc2)) / d
        big = np.maximum(np.abs(p0), np.abs(ref[0])).astype(np.float32)
        ulp = np.spacing(np.abs(big)).astype(np.float64)
        bar_p = 4 * U * np.abs(p0 * lr * float(wd)) + Uu * (8 * U + r) + 1.5 * ulp
    return bar_p, bar_m, bar_v


def _check(got, ref, bars, what, keep=None, before=None):
    """got: float32 (p, m, v) of the kernel; ref: float64 (p, m, v); bars: (p, m, v).  ``keep``: elements whose moments must be
    ``before``'s bit for bit."""
    for name, k, r, b in zip("pmv", got, ref, bars):
        k = np.asarray(k, np.float64)
        nan_k, nan_r = np.isnan(k), np.isnan(r)
        assert np.array_equal(nan_k, nan_r), (what, name, "NaN at", np.flatnonzero(nan_k ^ nan_r)[:8])
        inf_k, inf_r = np.isinf(k), np.isinf(r)
        assert np.array_equal(inf_k, inf_r) and np.array_equal(k[inf_k], r[inf_r]), (what, name, "inf at", np.flatnonzero(inf_k ^ inf_r)[:8])
        ok = ~(nan_r | inf_r)
        if not ok.any():
            continue
        err = np.abs(k[ok] - r[ok])
        bb = b[ok]
        bad = ~(err <= bb)
        if bad.any():
            i = np.flatnonzero(ok)[np.flatnonzero(bad)[:5]]
            raise AssertionError(f"{what}: {name} off by more than its bar at elements {i.tolist()}: kernel {k[i].tolist()}, "
                                 f"float64 {r[i].tolist()}, bar {b[i].tolist()}")
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(bb > 0, err / bb, 0.0)
        _WORST[name] = max(_WORST[name], float(q.max()))
    if keep is not None and keep.any():
        for name, k, b0 in zip("mv", got[1:], before):
            assert np.array_equal(np.asarray(k)[keep].view(np.uint32), np.asarray(b0)[keep].view(np.uint32)), (what, name, "touched")


# ---------------------------------------------------------------------------------------------------------------- a seeded matrix
SIZES = [1, 3, 4, 5, 1023, 2097151, 2097152, 2097153, 3 * 2 ** 21 + 3]
PATTERNS = [(48, 3), (12, 5), (6, 1)]
# active parts per pattern: SH degrees 0-2 of the (P,16,3) record; a part of the (12, 5) period; (6, 1) is no multiple of 4 -- the
# degree-aware shortcut must stay off there, and its inactive elements take the full update (zero gradients and moments)
ACTIVE = {(48, 3): [3, 12, 27], (12, 5): [4, 7], (6, 1): [3]}


def _magnitudes(rng, n, lo):
    return np.exp(rng.uniform(math.log(lo), math.log(1e3), n))


def _case(seed):
    """One sampled case: a dict of everything a moss_adamw_flat_ex call takes, as host arrays."""
    rng = np.random.default_rng(1000 + seed)
    big = seed % 40 == 0                                     # (a few cases at the grid-stride sizes: the CPU reference is the cost)
    n = SIZES[5 + (seed // 40) % 4] if big else int(rng.choice(SIZES[:5] + [int(rng.integers(6, 5000))]))
    aware = rng.random() < 0.4
    if aware and n < 1023:
        n = int(rng.integers(1023, 5000))                    # (room for whole periods)
    first = 4 * int(rng.integers(1, 64)) if rng.random() < 0.3 else 0
    eps = float(rng.choice([0.0, 1e-15, 1e-8]))
    wd = float(rng.choice([0.0, 0.01, 0.01]))
    beta1, beta2 = [(0.9, 0.999), (0.8, 0.99)][int(rng.integers(2))]
    step = int(rng.choice([1, 2, 1000, 3000]))
    # segments: 1-8, ends (global) at every residue mod 4, some 1-3 elements long; the last one ends at the end of the range
    nseg = int(rng.integers(1, 9)) if n > 8 else int(rng.integers(1, n + 1))
    cuts = set()
    while len(cuts) < nseg - 1:
        c = int(rng.integers(1, n))
        cuts.add(c)
        if len(cuts) < nseg - 1 and rng.random() < 0.3 and c + 3 < n:
            cuts.add(c + int(rng.integers(1, 4)))           # a segment of 1-3 elements
    if aware and rng.random() < 0.6:                         # (segments on float4 boundaries: where the degree-aware shortcut applies)
        cuts = {c - c % 4 for c in cuts if c >= 4}
    ends = [first + c for c in sorted(cuts)] + [first + n]
    nseg = len(ends)
    lr = (np.exp(rng.uniform(math.log(1e-4), math.log(5e-2), nseg))).astype(np.float32)
    period, split, lr2, active = [0] * nseg, [0] * nseg, [0.0] * nseg, [0] * nseg
    for s in range(nseg):
        if rng.random() < (0.7 if aware else 0.5):
            pat = PATTERNS[int(rng.integers(3))]
            period[s], split[s], lr2[s] = pat[0], pat[1], float(lr[s] / 20)
            if aware:
                active[s] = int(rng.choice(ACTIVE[pat]))
    inactive_zero = int(aware and rng.random() < 0.5)
    nextra = int(rng.integers(0, 4))
    scale = float(rng.choice([1.0, 0.5, 1.0 / 3.0]))
    lo = 1e-12 if eps == 0.0 else 1e-30                      # (eps = 0: a g^2 that underflows would divide by zero -- in float32 only)
    sgn = lambda k: np.where(rng.random(k) < 0.5, -1.0, 1.0)
    g = (sgn(n) * _magnitudes(rng, n, lo)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0.0
    g[rng.random(n) < 0.05] = -0.0
    extra = [(sgn(n) * _magnitudes(rng, n, lo)).astype(np.float32) for _ in range(nextra)]
    if rng.random() < 0.3 and n >= 8:                        # NaN / inf in one element of a float4: only that element may go bad
        for val in (np.nan, np.inf, -np.inf):                # (one landing on an inactive element is zeroed below: never read)
            (extra[0] if extra and rng.random() < 0.5 else g)[int(rng.integers(n))] = val
    p = (rng.standard_normal(n) * _magnitudes(rng, n, 1e-6)).astype(np.float32)
    if step == 1:
        m = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
    else:
        sc = _magnitudes(rng, n, lo)
        m = (sgn(n) * sc * 0.3).astype(np.float32); v = (sc * sc * rng.uniform(0.1, 1.0, n)).astype(np.float32)
    ina = oracle.adamw_inactive_per_element(first, n, ends, period, active) if aware else np.zeros(n, bool)
    if ina.any():
        # the contract: inactive elements have zero moments and zero gradients, except in the float4 that hold no active element where
        # the shortcut applies (segment starting on a float4, period a multiple of 4, eps > 0) -- those are never read
        m[ina] = 0.0; v[ina] = 0.0; g[ina] = 0.0
        for e in extra:
            e[ina] = 0.0
        if inactive_zero:
            p[ina] = 0.0
        if eps > 0:
            j = np.arange(first, first + n)
            starts = [0] + ends[:-1]
            skip = np.zeros(n, bool)
            for s in range(nseg):
                if active[s] and period[s] % 4 == 0 and starts[s] % 4 == 0:
                    # (the float4 of j starts at j - j % 4, inside the segment, at ph - ph % 4 of the period)
                    ph = (j - starts[s]) % period[s]
                    skip |= (j >= starts[s]) & (j - j % 4 + 3 < ends[s]) & (ph - ph % 4 >= (active[s] + 3) // 4 * 4)
            g[skip] = 123.0
            for e in extra:
                e[skip] = -7.0
    return dict(n=n, first=first, eps=eps, wd=wd, beta1=beta1, beta2=beta2, step=step, ends=ends, lr=lr, period=period, split=split,
                lr2=np.array(lr2, np.float32), active=active, aware=aware, inactive_zero=inactive_zero, scale=scale, p=p, g=g, m=m,
                v=v, extra=extra, inactive=ina)


class _Flat:
    """A moss_adamw_flat_ex call over device copies of a case's arrays (the ctypes arrays are kept alive with it)."""

    def __init__(self, gpu, c, step_state=None):
        from moss_amd import _lib
        self.L = _lib.lib()
        self.dev = {k: torch.from_numpy(c[k]).to(gpu) for k in ("p", "g", "m", "v")}
        self.extra = [torch.from_numpy(e).to(gpu) for e in c["extra"]]
        nseg = len(c["ends"])
        self.ends = (C.c_longlong * nseg)(*c["ends"])
        self.lr = (C.c_float * nseg)(*[float(x) for x in c["lr"]])
        self.per = (C.c_int * nseg)(*c["period"]); self.spl = (C.c_int * nseg)(*c["split"])
        self.lr2 = (C.c_float * nseg)(*[float(x) for x in c["lr2"]]); self.act = (C.c_int * nseg)(*c["active"])
        a = self.a = _lib.AdamWFlatArgs()
        a.first, a.count = c["first"], c["n"]
        a.params, a.grads, a.exp_avg, a.exp_avg_sq = (self.dev[k].data_ptr() for k in ("p", "g", "m", "v"))
        a.num_segments, a.segment_end, a.segment_lr = nseg, C.addressof(self.ends), C.addressof(self.lr)
        a.segment_period, a.segment_split, a.segment_lr2 = C.addressof(self.per), C.addressof(self.spl), C.addressof(self.lr2)
        a.segment_active = C.addressof(self.act) if c["aware"] else None
        a.inactive_zero = c["inactive_zero"]
        a.beta1, a.beta2, a.eps, a.weight_decay = c["beta1"], c["beta2"], c["eps"], c["wd"]
        a.step = c["step"]
        a.step_state = None if step_state is None else step_state.data_ptr()
        a.num_grads_extra, a.grad_scale = len(self.extra), c["scale"]
        for i, e in enumerate(self.extra):
            a.grads_extra[i] = e.data_ptr()

    def __call__(self, gpu):
        rc = self.L.moss_adamw_flat_ex(C.addressof(self.a), torch.cuda.current_stream(gpu).cuda_stream)
        assert rc == 0, rc

    def state(self):
        return tuple(self.dev[k].cpu().numpy() for k in ("p", "m", "v"))


def _reference(c, p, g, m, v, step, lr=None):
    """float64 (p, m, v) and the bars for one step of case ``c`` from the float32 state (p, g, m, v) before it."""
    n = c["n"]
    if lr is None:
        lr = oracle.adamw_lr_per_element(c["first"], n, c["ends"], c["lr"], c["period"], c["split"], c["lr2"])
    geff = oracle.adamw_grad_sum_f32(g, c["extra"], c["scale"])
    geff = np.where(c["inactive"], np.float32(0.0), geff)    # (an inactive element's gradient is not part of the step)
    ref = oracle.adamw_step_f64(p, geff, m, v, lr, c["beta1"], c["beta2"], c["eps"], c["wd"], step)
    return ref, _bars(p, geff, m, v, lr, c["beta1"], c["beta2"], c["eps"], c["wd"], step, ref)


def test_flat_adamw_matrix_against_float64(gpu, hip_lib):
    """240 sampled cases of the flat update (module docstring): sizes around the grid-stride threshold, 1-8 segments with ends at every
    residue mod 4 and of 1-3 elements, periodic rates (48, 3) / (12, 5) / (6, 1), shards, 0-3 extra gradient buffers, the degree-aware
    form at SH degrees 0-2 with and without known-zero parameters, host steps 1 / 2 / 1000 / 3000, eps 0 / 1e-15 / 1e-8, weight decay
    0 / 0.01, two beta pairs, gradients from 1e-30 to 1e3 with zeros, -0, NaN and inf."""
    for seed in range(240):
        c = _case(seed)
        f = _Flat(gpu, c)
        f(gpu)
        got = f.state()
        ref, bars = _reference(c, c["p"], c["g"], c["m"], c["v"], c["step"])
        what = {k: c[k] for k in ("n", "first", "ends", "period", "active", "aware", "inactive_zero", "eps", "wd", "step")}
        _check(got, ref, bars, f"case {seed} {what}", keep=c["inactive"], before=(c["m"], c["v"]))
        del f
    torch.cuda.synchronize(gpu)


def test_flat_adamw_refuses_misaligned_arrays(gpu, hip_lib):
    """The kernel moves float4: every array -- extra gradient buffers too -- must start on 16 bytes, like moss_adamw_multi's."""
    c = _case(3)
    c["extra"] = [c["g"].copy()]
    f = _Flat(gpu, c)
    a = f.a
    L = f.L
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for field in ("params", "grads", "exp_avg", "exp_avg_sq"):
        ok = getattr(a, field)
        setattr(a, field, ok + 4)
        assert L.moss_adamw_flat_ex(C.addressof(a), stream) == -1, field
        setattr(a, field, ok)
    ok = a.grads_extra[0]
    a.grads_extra[0] = ok + 4
    assert L.moss_adamw_flat_ex(C.addressof(a), stream) == -1
    a.grads_extra[0] = ok
    before = f.state()
    torch.cuda.synchronize(gpu)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, (c["p"], c["m"], c["v"])))
    f(gpu)                                                    # (and the aligned call runs)


# ---------------------------------------------------------------------------------------------------- the device-side step counter
def test_flat_adamw_device_step_counter_and_rate_table_over_3000_steps(gpu, hip_lib):
    """3000 capturable steps on ONE step-state block, launches of 1, 31, 32, 33 and 2048 blocks in turn (the count changes between calls,
    as densification changes it): the counter is right after every call, the two-level completion counters come back to zero, the bias
    corrections and the device-side learning rates (the launch arguments say otherwise) match float64 at sampled steps, and a guarded
    call leaves parameters, moments and the whole state block bit for bit."""
    from moss_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(7)
    N = 2048 * 1024 + 5
    counts = [1021, 31 * 1024 - 3, 32 * 1024, 33 * 1024 - 1, N]         # 1, 31, 32, 33 and 2048 blocks of 256 threads x 4 elements
    ends = [5, 1000, 40001, N]                                          # (a short first segment, ends at residues 1, 0, 1, 1)
    c = dict(n=N, first=0, eps=1e-15, wd=0.01, beta1=0.9, beta2=0.999, step=1, ends=ends,
             lr=np.float32([1e3, 1e3, 1e3, 1e3]), period=[0, 48, 0, 0], split=[0, 3, 0, 0], lr2=np.float32([1e3] * 4), active=[0] * 4,
             aware=False, inactive_zero=0, scale=1.0, p=rng.standard_normal(N).astype(np.float32), g=np.zeros(N, np.float32),
             m=np.zeros(N, np.float32), v=np.zeros(N, np.float32), extra=[], inactive=np.zeros(N, bool))
    state = torch.zeros(int(L.moss_adamw_state_bytes()) // 4, dtype=torch.int32, device=gpu)
    table_lr, table_lr2 = np.float32([1.6e-4, 2.5e-3, 5e-2, 1e-3]), np.float32([0, 1.25e-4, 0, 0])
    sf = state.view(torch.float32)
    state[12] = 1
    sf[16:20] = torch.from_numpy(table_lr).to(gpu); sf[24:28] = torch.from_numpy(table_lr2).to(gpu)
    f = _Flat(gpu, c, step_state=state)
    grads = [torch.from_numpy((rng.standard_normal(N) * 10.0 ** rng.uniform(-3, 1, N)).astype(np.float32)).to(gpu) for _ in range(3)]
    skip = torch.zeros(1, dtype=torch.int32, device=gpu)
    checks = {1, 2, 3, 31, 32, 33, 34, 35, 999, 1000, 2047, 2048, 2998, 2999, 3000}
    lr_full = oracle.adamw_lr_per_element(0, N, ends, table_lr, c["period"], c["split"], table_lr2)
    for t in range(1, 3001):
        n = counts[t % len(counts)]
        f.a.count = n
        f.a.grads = grads[t % 3].data_ptr()
        if t in (2, 1000, 2999):                             # a guarded call first: a no-op
            f.a.skip_word, f.a.skip_mask = skip.data_ptr(), 2
            skip.fill_(2)
            before = (f.state(), state.clone())
            f(gpu)
            after = (f.state(), state.clone())
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before[0], after[0])) and torch.equal(before[1], after[1]), t
            skip.fill_(0)                                    # ... and the guarded call of the step itself runs
        if t in checks:
            p0, m0, v0 = (x[:n] for x in f.state())
            g0 = grads[t % 3][:n].cpu().numpy()
        f(gpu)
        f.a.skip_word, f.a.skip_mask = None, 0
        assert int(state[0]) == t, (t, int(state[0]))
        if t in checks:
            assert int(state[64]) == 0 and not bool(state[128::64][:32].any()), t           # completion counters back to zero
            cc = dict(c, n=n, extra=[], inactive=np.zeros(n, bool))
            ref, bars = _reference(cc, p0, g0, m0, v0, t, lr=lr_full[:n])
            got = tuple(x[:n] for x in f.state())
            _check(got, ref, bars, f"device step {t} ({n} elements)")


# ---------------------------------------------------------------------------------------------------------------- moss_adamw_multi
def test_adamw_multi_against_float64(gpu, hip_lib):
    """moss_adamw_multi over 1-8 tensors of 0, 1, 3, 4, 5, 1023 and 1 048 577 elements (past one tensor's 1024-block grid stride) with
    step counts 1, 7 and 3000 of their own: every element against float64, the same bars."""
    from moss_amd import _lib
    L = _lib.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    sizes = [0, 1, 3, 4, 5, 1023, 1048577]
    for seed in range(12):
        rng = np.random.default_rng(500 + seed)
        k = int(rng.integers(1, 9))
        ns = [int(rng.choice(sizes)) for _ in range(k)]
        if seed < 2:
            ns[0] = 1048577
        steps = [int(rng.choice([1, 7, 3000])) for _ in range(k)]
        lrs = np.exp(rng.uniform(math.log(1e-4), math.log(5e-2), k)).astype(np.float32)
        beta1, beta2 = [(0.9, 0.999), (0.8, 0.99)][seed % 2]
        eps, wd = [1e-15, 1e-8, 0.0][seed % 3], [0.01, 0.0][(seed // 2) % 2]
        lo = 1e-12 if eps == 0.0 else 1e-30
        host = []
        for n, t in zip(ns, steps):
            sc = np.exp(rng.uniform(math.log(lo), math.log(1e3), n))
            g = (np.where(rng.random(n) < 0.5, -1, 1) * sc).astype(np.float32)
            p = (rng.standard_normal(n) * np.exp(rng.uniform(math.log(1e-6), math.log(1e3), n))).astype(np.float32)
            m = np.zeros(n, np.float32) if t == 1 else (rng.standard_normal(n) * sc * 0.3).astype(np.float32)
            v = np.zeros(n, np.float32) if t == 1 else (sc * sc * rng.uniform(0.1, 1, n)).astype(np.float32)
            host.append((p, g, m, v))
        dev = [[torch.from_numpy(x).to(gpu) if x.size else torch.zeros(4, device=gpu) for x in h] for h in host]
        a = _lib.AdamWMultiArgs()
        a.num_tensors = k
        a.beta1, a.beta2, a.eps, a.weight_decay = beta1, beta2, eps, wd
        for i in range(k):
            a.numel[i], a.lr[i], a.step[i] = ns[i], float(lrs[i]), steps[i]
            a.params[i], a.grads[i], a.exp_avg[i], a.exp_avg_sq[i] = (t.data_ptr() for t in dev[i])
        assert L.moss_adamw_multi(C.addressof(a), stream) == 0
        for i in range(k):
            if ns[i] == 0:
                continue
            p, g, m, v = host[i]
            ref = oracle.adamw_step_f64(p, g, m, v, lrs[i], beta1, beta2, eps, wd, steps[i])
            bars = _bars(p, g, m, v, lrs[i], beta1, beta2, eps, wd, steps[i], ref)
            got = (dev[i][0].cpu().numpy(), dev[i][2].cpu().numpy(), dev[i][3].cpu().numpy())
            _check(got, ref, bars, f"multi seed {seed} tensor {i} (n {ns[i]}, step {steps[i]})")


# ------------------------------------------------------------------------------------------------------------ 4 GB per array and more
def test_flat_adamw_beyond_4gb_per_array(gpu, hip_lib):
    """ONE moss_adamw_flat_ex call at 2^30 + 4099 elements per array (five arrays of 4.3 GB: parameters, gradients, both moments, one
    extra gradient buffer), two segments, step 2 with non-zero moments: the first 4096 elements, the window around the 0xffffff00-byte
    end of a 32-bit buffer record, the last 4099 and a million random elements against float64."""
    n = 2 ** 30 + 4099
    need = 5 * 4 * n
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 1.25 * need:
        pytest.skip(f"needs {1.25 * need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")
    from moss_amd import _lib
    L = _lib.lib()
    gen = torch.Generator(device=gpu).manual_seed(11)
    p = torch.randn(n, device=gpu, generator=gen)
    g = torch.randn(n, device=gpu, generator=gen)
    e = torch.randn(n, device=gpu, generator=gen)
    m = torch.randn(n, device=gpu, generator=gen).mul_(0.1)
    v = torch.rand(n, device=gpu, generator=gen).mul_(0.01)
    idx = np.unique(np.concatenate([np.arange(4096), np.arange(2 ** 30 - 4096, 2 ** 30 + 4096), np.arange(n - 4099, n),
                                    np.random.default_rng(3).integers(0, n, 10 ** 6)]))
    it = torch.from_numpy(idx).to(gpu)
    before = [t[it].cpu().numpy() for t in (p, g, e, m, v)]
    ends = (C.c_longlong * 2)(2 ** 29 + 3, n)
    lrs = (C.c_float * 2)(1e-3, 5e-2)
    a = _lib.AdamWFlatArgs()
    a.first, a.count = 0, n
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
    a.num_segments, a.segment_end, a.segment_lr = 2, C.addressof(ends), C.addressof(lrs)
    a.beta1, a.beta2, a.eps, a.weight_decay, a.step = 0.9, 0.999, 1e-8, 0.01, 2
    a.num_grads_extra, a.grad_scale = 1, 0.5
    a.grads_extra[0] = e.data_ptr()
    assert L.moss_adamw_flat_ex(C.addressof(a), torch.cuda.current_stream(gpu).cuda_stream) == 0
    got = [t[it].cpu().numpy() for t in (p, m, v)]
    del p, g, e, m, v, it
    torch.cuda.empty_cache()
    lr = np.where(idx < 2 ** 29 + 3, np.float32(1e-3), np.float32(5e-2))
    geff = oracle.adamw_grad_sum_f32(before[1], [before[2]], 0.5)
    ref = oracle.adamw_step_f64(before[0], geff, before[3], before[4], lr, 0.9, 0.999, 1e-8, 0.01, 2)
    bars = _bars(before[0], geff, before[3], before[4], lr, 0.9, 0.999, 1e-8, 0.01, 2, ref)
    _check(got, ref, bars, "2^30 + 4099 elements")
