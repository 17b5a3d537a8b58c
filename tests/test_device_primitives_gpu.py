"""The device-only forms of the math primitives, each probed as itself on the GPU (tests/device_probe.py) and held to the
bound the code states for it: og_sin_turns is v_sin_f32, div_near / div_rcp / the PolyBLEP rdt are v_rcp_f32 plus one Newton
step, the fract family is v_fract_f32, clampf is v_med3_f32, tpt_update_coefficients_iq branches on a wave-uniform __any.
The host simulator replaces every one of them, and whole-voice parity at 1e-5 cannot tell 1 ulp from 30.

Every case prints its observed worst error and passes it to observed.note (profiles/device_primitives.md holds the record).
The argument builders are plain functions: tests/test_device_primitives_cpu.py checks on the CPU that they contain the edge
sets the assertions here call non-empty."""
import functools

import numpy as np
import pytest

from tests import device_probe as dp
from tests import observed

pytestmark = pytest.mark.gpu
f32 = np.float32
hexf = float.fromhex


def report(what, value, error=True):
    """print a figure; an observed worst ERROR also goes to observed.note (counts, shares and distances in ulp do not: the
    record of observed errors is condensed by its maximum)"""
    print("%-58s %.6g" % (what, value))
    if error:
        observed.note(value, tag=what)


def worst_difference(got, ref):
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return float(np.max(d[np.isfinite(d)], initial=0.0))


def concat_sets(sets):
    """{name: (base patterns, stride)} -> bases, strides of all voices and the slice of every set"""
    bases, strides, where, at = [], [], {}, 0
    for name, (b, s) in sets.items():
        b = np.atleast_1d(np.asarray(b)).astype(np.uint64)
        bases.append(b)
        strides.append(np.broadcast_to(np.asarray(s, dtype=np.uint64), b.shape))
        where[name] = slice(at, at + len(b))
        at += len(b)
    return np.concatenate(bases), np.concatenate(strides), where


# a walk of 256 steps from pattern 0 / 0x80000000: +-0 and the smallest denormals; from 0x007fff80: the largest denormals, the
# smallest normal (step 128) and its neighbours
ZERO_AND_DENORMALS = np.array([0x00000000, 0x80000000, 0x007FFF80, 0x807FFF80], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# sines
# ---------------------------------------------------------------------------------------------------------------------
def sine_arguments():
    quarter = np.arange(-64, 65)
    quarter = (quarter[quarter != 0] * 0.25).astype(f32)
    return {
        "pm64": (dp.bits(np.linspace(-64.0, 64.0, 1024)), 97),            # og_sinf, dense
        "pm1e5": (dp.bits(np.linspace(-1.0e5, 1.0e5, 256)), 1009),        # og_sinf, sparse
        "turns16": (dp.bits(np.linspace(-16.0, 16.0, 512)), 257),         # the FM range, in turns
        "turns2e6": (dp.bits(np.linspace(-2.0e6, 2.0e6, 256)), 3),        # |2t| < 2^22: the magic-number rounding still holds
        "unit": (dp.bits(np.linspace(-1.0, 2.0, 768, endpoint=False)), 127),  # [-1, 2) dense
        "quarters": (dp.around(quarter, 128), 1),                         # the exact points k/4 (step 128) and their neighbours
        "zero": (ZERO_AND_DENORMALS, 1),
    }


@functools.lru_cache(maxsize=None)
def sine_sweep():
    a, sa, where = concat_sets(sine_arguments())
    r = dp.probe("sine", 1024).run(a, sa)
    assert np.array_equal(dp.bits(r["out"][:, :, 3]), dp.bits(r["x"]))  # the lanes formed the arguments the host formed
    return r, where


def tangent_arguments():
    """the first quadrant dense, +-0 and denormals, and what the TPT cases form: x and the complement pi/2 - x"""
    xs = [np.array([0.0, -0.0], dtype=f32)]
    for sr in dp.TPT_RATES:
        s = dp.tpt_slots(sr)
        x = dp.tpt_x(dp.tpt_cutoffs(sr), s)
        xs += [x, ((f32(hexf("0x1.921fb6p+0")) - x).astype(f32) + f32(hexf("-0x1.777a5cp-25"))).astype(f32)]
    return {"q1": (dp.bits(np.linspace(1.0e-4, 1.5707, 1024)), 47), "zero": (ZERO_AND_DENORMALS, 1)}, np.unique(np.concatenate(xs))


@functools.lru_cache(maxsize=None)
def tangent_sweep():
    sets, pts = tangent_arguments()
    a, sa, where = concat_sets(sets)
    p = dp.probe("tangent", 1024)
    r, q = p.run(a, sa), p.points(pts)
    x = np.concatenate([r["x"].ravel(), q["x"]])
    out = np.concatenate([r["out"].reshape(-1, 4), q["out"]])
    assert np.array_equal(dp.bits(out[:, 3]), dp.bits(x))
    return x, out


def test_ieee_only_helpers_give_the_bits_of_the_host_build():
    """og_sinf, og_sin_turns_poly, og_tan_poly and og_tanf_q1 hold only IEEE mul / add / fmaf and a correctly rounded
    divide under -ffp-contract=off: the device must give the bits g++ gives for the same text."""
    r, where = sine_sweep()
    host = dp.host_eval("sine", r["x"]).reshape(r["out"].shape)
    for col, name in ((0, "og_sinf"), (1, "og_sin_turns_poly")):
        bad = dp.bits(host[:, :, col]) != dp.bits(r["out"][:, :, col])
        report("%s: arguments whose bits differ from the host build" % name, bad.sum(), error=False)
        report("%s: worst difference from the host build" % name, worst_difference(r["out"][:, :, col], host[:, :, col]))
        assert not bad.any(), (name, r["x"][bad][:8], r["out"][:, :, col][bad][:8], host[:, :, col][bad][:8])
    x, out = tangent_sweep()
    host = dp.host_eval("tangent", x)
    for col, name in ((0, "og_tan_poly"), (1, "og_tanf_q1")):
        ok = np.isfinite(host[:, col])  # (1 / tan_poly(pi/2 - x) beyond the quadrant: nobody's domain)
        bad = (dp.bits(host[:, col]) != dp.bits(out[:, col])) & ok
        report("%s: arguments whose bits differ from the host build" % name, bad.sum(), error=False)
        report("%s: worst difference from the host build" % name, worst_difference(out[ok, col], host[ok, col]))
        assert not bad.any(), (name, x[bad][:8], out[bad, col][:8], host[bad, col][:8])
    assert len(x) > 250000 and r["x"].size > 700000


def test_hardware_sine_against_the_sine_of_the_fractional_part():
    """og_sin_turns = v_sin_f32 against sin(2 pi frac(t)) in f64.  The limit is the amplitude the host simulator's stand-in
    injects (og_math.h, OG_HOSTSIM branch: 1.1e-7) plus the final rounding 2^-25: the simulator is what lets the GPU tests
    count in the CPU suite, so the hardware must not be worse than it.  (The stand-in itself misses this limit where its sum
    passes 1.0 and rounds with the ulp above 1 -- 1.7e-7 at the quarter turns; the instruction does not, 5.9e-8 there.)"""
    r, where = sine_sweep()
    limit = 1.1e-7 + 2.0 ** -25
    worst = 0.0
    for name in ("unit", "turns16", "quarters", "zero"):
        t = r["x"][where[name]].astype(np.float64)
        got = r["out"][where[name]][:, :, 2]
        err = float(np.max(np.abs(got - np.sin(2.0 * np.pi * (t - np.floor(t))))))
        report("og_sin_turns, %s: worst absolute error" % name, err)
        worst = max(worst, err)
    t = r["x"][where["quarters"]][:, 128]
    assert np.array_equal(t * f32(4.0), np.round(t * f32(4.0))) and len(t) == 128
    assert np.isfinite(r["out"][:, :, 2]).all()
    assert worst <= limit, (worst, limit)


def exact_arguments():
    """|x| < 120: 2^19 arguments spread geometrically (a walk over bit patterns from 1e-8 up) and 2^19 uniformly, both signs;
    then 64 floats either side of +-pi/4, +-2^-12, +-120 and +-k pi/2 for k = 1 .. 76, and +-0"""
    b0, b1 = int(dp.bits(f32(1.0e-8))[0]), int(dp.bits(f32(120.0))[0])
    step = (b1 - b0) // (2048 * 256)
    geo = b0 + np.arange(2048, dtype=np.uint64) * np.uint64(256 * step)
    geo[1::2] |= np.uint64(0x80000000)
    uni = dp.bits(np.linspace(-119.88, 119.88, 2048)).astype(np.uint64)
    edges = np.concatenate([[np.pi / 4, 2.0 ** -12, 120.0], np.arange(1, 77) * (np.pi / 2)]).astype(f32)
    edges = np.concatenate([edges, -edges])
    return {"geometric": (geo, step), "uniform": (uni, 59)}, {"edges": (dp.around(edges, 64), 1), "zero": (ZERO_AND_DENORMALS[:2], 1)}


def test_exact_sine_and_cosine_give_the_bits_of_the_host_libm():
    """og_sinf_exact / og_cosf_exact restate glibc's sincosf (its FMA build); on the device they must give the host libm's
    bits for every |x| < 120.  From 120 on the device form returns NaN by design (no caller gets there)."""
    if not dp.host_has_fma():
        pytest.skip("host CPU without FMA: glibc uses its non-FMA sincosf build")
    bulk, edge = exact_arguments()
    p = dp.probe("exact", 4096)
    a, sa, _ = concat_sets(bulk)
    r = p.run(a, sa)
    a, sa, _ = concat_sets(edge)
    e = p.run(a, sa, frames=129)
    x = np.concatenate([r["x"].ravel(), e["x"].ravel()])
    out = np.concatenate([r["out"].reshape(-1, 4), e["out"].reshape(-1, 4)])
    inside = np.abs(x) < f32(120.0)
    assert inside.sum() >= 1000000 and (~inside).sum() >= 128
    for col, fn in ((0, "sinf"), (1, "cosf")):
        ref = dp.host_libm(fn, x)
        bad = (dp.bits(ref) != dp.bits(out[:, col])) & inside
        report("og_%s_exact: arguments below 120 whose bits differ from libm" % fn, bad.sum(), error=False)
        report("og_%s_exact: worst difference from libm below 120" % fn, worst_difference(out[inside, col], ref[inside]))
        assert not bad.any(), (fn, x[bad][:8], out[bad, col][:8], ref[bad][:8])
        beyond = out[~inside, col]  # from 120 on the device form is NaN by design; a host compilation of it asks libm
        assert (np.isnan(beyond) | (dp.bits(beyond) == dp.bits(ref[~inside]))).all()


# ---------------------------------------------------------------------------------------------------------------------
# quotients
# ---------------------------------------------------------------------------------------------------------------------
def divide_arguments():
    """(a, b) walks.  documented: b over [1, 2^40] and a over every finite magnitude of both signs (a multiplicative walk
    over all bit patterns; the non-finite ones are dropped);  blep: b = dt over (EPSILON, 1], a = t or t - 1 in [-1, 1]"""
    v = np.arange(4096, dtype=np.uint64)
    one, top, eps = int(dp.bits(f32(1.0))[0]), int(dp.bits(f32(2.0 ** 40))[0]), int(dp.bits(dp.EPSILON)[0])
    sb = (top - one) // (4096 * 256)
    doc = dict(a=(v * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF), sa=0x85EBCA6B, b=one + v * np.uint64(256 * sb), sb=sb)
    doc_top = dict(a=doc["a"][:256], sa=0x85EBCA6B, b=np.full(256, top - 255, dtype=np.uint64), sb=1)  # ... up to 2^40 itself
    sb = (one - eps) // (4096 * 256)
    rng = np.random.default_rng(5)
    blep = dict(a=dp.bits(rng.uniform(-1.0, 1.0, 4096).astype(f32) * f32(0.8)).astype(np.uint64), sa=12345,
                b=eps + 1 + v * np.uint64(256 * sb), sb=sb)
    return {"documented": doc, "documented_top": doc_top, "blep": blep}


def tpt_denominators():
    """1 + f / q + f * f over the TPT cases, f from the host build of the tangent (the device gives its bits)"""
    out = []
    for sr in dp.TPT_RATES:
        s = dp.tpt_slots(sr)
        x = dp.tpt_x(dp.tpt_cutoffs(sr), s)
        f = ((s["two_sr"] * dp.host_eval("tangent", x)[:, 1]).astype(f32) * s["period"]).astype(f32)
        for q in dp.TPT_QS:
            inv_q = np.full(len(f), f32(1.0) / f32(q), dtype=f32)
            out.append(dp.host_libm("fmaf", f, f, dp.host_libm("fmaf", inv_q, f, np.ones(len(f), dtype=f32))))
    return np.concatenate(out)


def relative(got, ref):
    """worst |got - ref| / |ref| over the normal, non-zero quotients"""
    m = np.abs(ref) >= f32(1.1754944e-38)
    return float(np.max(np.abs(got[m].astype(np.float64) - ref[m]) / np.abs(ref[m].astype(np.float64)), initial=0.0))


def test_reciprocal_quotients_are_within_an_ulp_of_the_ieee_quotient():
    """div_near(a, b) and div_rcp(a, b, rcp(b)) against numpy's f32 quotient: 1 ulp of the correctly rounded quotient, the
    comment's own claim -- on the documented domain (b in [1, 2^40], finite a) and on the domains actually used: 1 / (1 + f/q
    + f^2) and 1 / og_tan_poly(y) of the TPT coefficient forms (y down to the small negative one at Nyquist), t / dt and
    (t - 1) / dt of PolyBLEP with dt in (EPSILON, 1].  The share of results that are not correctly rounded is recorded."""
    p = dp.probe("divide", 4096)
    worst = 0
    for name, s in divide_arguments().items():
        r = p.run(s["a"], s["sa"], s["b"], s["sb"])
        a, b = r["x"].ravel(), r["y"].ravel()
        ok = np.isfinite(a)
        a, b, out = a[ok], b[ok], r["out"].reshape(-1, 4)[ok]
        if name.startswith("documented"):
            assert b.min() >= 1.0 and b.max() <= 2.0 ** 40 and (a < 0).any() and (a > 0).any()
            assert np.abs(a).min() < 1e-37 and np.abs(a).max() > 1e37
        else:
            assert b.min() > dp.EPSILON and b.max() <= 1.0 and np.abs(a).max() <= 1.0
        with np.errstate(all="ignore"):
            ref = (a / b).astype(f32)
        for col, fn in ((0, "div_near"), (1, "div_rcp")):
            d = dp.ulp_distance(out[:, col], ref)
            report("%s, %s: worst distance from the IEEE quotient in ulp" % (fn, name), d.max(), error=False)
            report("%s, %s: share not correctly rounded" % (fn, name), float(np.mean(d != 0)), error=False)
            report("%s, %s: worst relative error against the IEEE quotient" % (fn, name), relative(out[:, col], ref))
            worst = max(worst, int(d.max()))
            assert d.max() <= 1, (fn, name, a[d > 1][:8], b[d > 1][:8], out[d > 1, col][:8], ref[d > 1][:8])
        assert name != "documented_top" or b.max() == 2.0 ** 40
    # a = 1: the denominators of h over the TPT cases ...
    b = tpt_denominators()
    r = p.points(np.ones(len(b), dtype=f32), b)
    d = dp.ulp_distance(r["out"][:, 0], (f32(1.0) / b).astype(f32))
    report("div_near(1, 1 + f/q + f^2): worst distance in ulp", d.max(), error=False)
    report("div_near(1, 1 + f/q + f^2): share not correctly rounded", float(np.mean(d != 0)), error=False)
    report("div_near(1, 1 + f/q + f^2): worst relative error", relative(r["out"][:, 0], (f32(1.0) / b).astype(f32)))
    assert d.max() <= 1 and b.min() >= 1.0 and b.max() > 1e13
    # ... and the flat form's 1 / og_tan_poly(y): y over the first quadrant and the complements the TPT cases form
    x, out = tangent_sweep()
    t0 = out[:, 0]
    ok = (np.abs(x) >= 1e-8) & (x <= 1.5707)  # (0, pi/4] is what the flat form passes, and the complement at Nyquist, -4.4e-8
    assert (x[ok] < 0).any() and (t0[ok] < 1).any() and (t0[ok] > 1).any()
    d = dp.ulp_distance(out[ok, 2], (f32(1.0) / t0[ok]).astype(f32))
    report("div_near(1, og_tan_poly(y)): worst distance in ulp", d.max(), error=False)
    report("div_near(1, og_tan_poly(y)): share not correctly rounded", float(np.mean(d != 0)), error=False)
    report("div_near(1, og_tan_poly(y)): worst relative error", relative(out[ok, 2], (f32(1.0) / t0[ok]).astype(f32)))
    assert d.max() <= 1, (x[ok][d > 1][:8], out[ok, 2][d > 1][:8])
    assert worst <= 1


# ---------------------------------------------------------------------------------------------------------------------
# fract, clamp
# ---------------------------------------------------------------------------------------------------------------------
TIE = f32(-2.0 ** -25)  # 1 + x rounds to 1.0 for TIE <= x < 0 (the tie itself goes to even): the reference returns 1.0 there


def fract_arguments():
    """[-4, 4] dense; +-(2^23 - 2 .. 2^24 + 2): both ends float by float and a walk between; whole numbers of both signs;
    denormals and +-0; the negative floats above -2^-26 sampled through every binade down to the denormals; 128 floats either
    side of -2^-25, -2^-24 and -2^-23.  (Every float of [-2^-23, 0) is visited by fract_every_float.)"""
    whole = np.arange(0, 1024).astype(f32)
    lo, hi = int(dp.bits(f32(2.0 ** 23 - 2))[0]), int(dp.bits(f32(2.0 ** 24 + 2))[0])
    big = np.concatenate([[lo, hi - 255], lo + 256 + np.arange(126, dtype=np.uint64) * np.uint64(256 * 259)]).astype(np.uint64)
    big_stride = np.concatenate([[1, 1], np.full(126, 259)])
    assert big[-1] + 255 * 259 < hi
    tiny_top = int(dp.bits(f32(2.0 ** -26))[0])
    tiny = 0x80000000 + np.arange(256, dtype=np.uint64) * np.uint64(tiny_top // 256)
    return {
        "dense": (dp.bits(np.linspace(-4.0, 4.0, 1024)), 4099),
        "big": (np.concatenate([big, big | np.uint64(0x80000000)]), np.concatenate([big_stride, big_stride])),
        "whole": (np.concatenate([dp.bits(whole), dp.bits(-whole)]), 0),
        "zero": (ZERO_AND_DENORMALS, 1),
        "tiny_negative": (tiny, tiny_top // 65536),
        "tie": (dp.around(np.array([TIE, -2.0 ** -24, -2.0 ** -23], dtype=f32), 128), 1),
    }


FRACT_CHUNK = 832  # floats per lane and frame: 4096 lanes x 256 frames x 832 = 0x34000000, the floats of [-2^-23, 0)


def fract_every_float():
    """bases and stride of the 4096 walks whose steps are the first patterns of consecutive chunks of FRACT_CHUNK floats,
    from the smallest negative denormal to -2^-23"""
    first, last = 0x80000001, int(dp.bits(f32(-2.0 ** -23))[0])
    assert last - first + 1 == 4096 * 256 * FRACT_CHUNK
    return first + np.arange(4096, dtype=np.uint64) * np.uint64(256 * FRACT_CHUNK), FRACT_CHUNK


def fract_check(x, out, phase):
    """one sweep against the Rust semantics.  Returns the counts of arguments where the reference gives 1.0 and of negative
    whole arguments and -0, and the worst difference; asserts that the device differs from the reference only as the
    comments say."""
    x, out = x.ravel(), out.reshape(-1, 4)
    floor_ref, keep_ref = dp.rem_euclid1(x), dp.fmod1(x)
    one = floor_ref == f32(1.0)
    assert np.array_equal(one, (x >= TIE) & (x < 0))
    neg_whole = np.signbit(x) & (x == np.trunc(x))  # negative whole numbers and -0
    cols = [(0, "fract_floor", floor_ref), (1, "wrap_phase", floor_ref), (2, "fract_keep_sign", keep_ref),
            (3, "fract_phase", floor_ref) if phase else (3, "fmod1", keep_ref)]
    worst = 0.0
    for col, name, ref in cols:
        got = out[:, col]
        worst = max(worst, worst_difference(got, ref))
        differs = ~dp.same_value(got, ref)
        if ref is floor_ref:
            assert np.array_equal(differs, one), (name, x[differs ^ one][:8], got[differs ^ one][:8])
            assert (dp.bits(got[one]) == 0x3F7FFFFF).all(), name  # 0.99999994, the clamp of v_fract_f32
        else:
            assert not differs.any(), (name, x[differs][:8], got[differs][:8], ref[differs][:8])
        sign = (dp.bits(got) != dp.bits(ref)) & ~differs  # a zero of the other sign
        assert not (sign & ~neg_whole).any(), (name, x[sign & ~neg_whole][:8])
        assert ((got >= 0) & (got < 1) | (ref is keep_ref)).all()
    return int(one.sum()), int(neg_whole.sum()), worst


def test_fract_family_against_the_rust_semantics():
    """fract_floor / wrap_phase / fract_phase against rem_euclid(1.0), fract_keep_sign / fmod1 against `% 1.0`, both written
    in numpy f32.  Equal as values (+0 = -0) everywhere except where the reference's r + 1.0 rounds up to 1.0 -- that is
    -2^-25 <= x < 0: the tie at -2^-25 goes to even -- where the device must return 0.99999994 (the comment in og_nodes.hip.h
    says -6e-8 < x < 0, which is loose: between -5.96e-8 and -2.98e-8 both sides give 0.99999994).  A zero result may
    differ in sign only for negative whole x and -0."""
    p = dp.probe("fract", 4096)
    a, sa, _ = concat_sets(fract_arguments())
    ones = wholes = points = 0
    worst = 0.0
    for phase in (0, 1):
        r = p.run(a, sa, sel=phase)
        n1, n2, w = fract_check(r["x"], r["out"], phase)
        ones, wholes, points, worst = ones + n1, wholes + n2, points + r["x"].size, max(worst, w)
    report("fract family against numpy: arguments", points, error=False)
    report("fract family against numpy: arguments where the reference gives 1.0 and the device 0.99999994", ones, error=False)
    report("fract family against numpy: negative whole arguments and -0", wholes, error=False)
    report("fract family against numpy: worst difference (0.99999994 for 1.0)", worst)
    assert ones > 60000 and wholes > 2048 and worst == 2.0 ** -24


def test_fract_family_on_every_float_of_the_last_negative_binades():
    """Every float of [-2^-23, 0) -- 872 415 232 of them, where the reference's r + 1.0 rounds -- compared on the device with
    the Rust semantics restated beside the helper (device_probe.BODIES["fract_all"]): no argument may differ, with 0.99999994
    for the reference's 1.0; and the reference's 1.0 must be counted on exactly the floats of [-2^-25, 0).  The restatement
    itself is held against numpy at the first float of every chunk."""
    a, chunk = fract_every_float()
    r = dp.probe("fract_all", 4096).run(a, chunk, c=dp.from_bits(np.full(len(a), chunk, dtype=np.uint32)))
    out = r["out"].astype(np.int64)
    report("fract family, every float of [-2^-23, 0): arguments", out.shape[0] * out.shape[1] * chunk, error=False)
    report("fract family, every float of [-2^-23, 0): fract_floor / wrap_phase / fract_phase differ", out[:, :, 0].sum())
    report("fract family, every float of [-2^-23, 0): fract_keep_sign / fmod1 differ", out[:, :, 1].sum())
    report("fract family, every float of [-2^-23, 0): reference 1.0, device 0.99999994", out[:, :, 2].sum(), error=False)
    assert np.array_equal(dp.bits(r["out"][:, :, 3]), dp.bits(dp.rem_euclid1(r["x"])))
    assert (r["out"][:, :, 3] == 1.0).any() and (r["out"][:, :, 3] < 1.0).any()
    assert out[:, :, 0].sum() == 0 and out[:, :, 1].sum() == 0
    assert out[:, :, 2].sum() == int(dp.bits(TIE)[0]) - 0x80000000  # the floats of [-2^-25, 0)


def clamp_arguments():
    tiny = f32(1.0e-45)
    inf = f32(np.inf)
    bounds = [(0.0, 1.0), (-1.0, 1.0), (20.0, 20000.0), (0.1, 10.0), (-0.7, 0.7), (0.0001, 0.9999), (5.0, 5.0), (0.0, 0.0),
              (-0.0, 0.0), (-inf, inf), (0.0, inf), (-inf, 0.0), (tiny, f32(3.0e-45)), (-tiny, tiny), (-3.0e38, 3.0e38)]
    xs, lo, hi = [], [], []
    for l, h in bounds:
        l, h = f32(l), f32(h)
        with np.errstate(invalid="ignore"):
            pts = [0.0, -0.0, inf, -inf, tiny, -tiny, f32(1.0e-40), f32(-1.0e-40), f32(1.0), f32(-1.0), f32(3.4e38), f32(-3.4e38),
                   l, h, f32(0.5) * l + f32(0.5) * h]
        for e in (l, h):
            pts += [np.nextafter(e, inf), np.nextafter(e, -inf)]
        pts = [v for v in pts if not np.isnan(v)]
        xs += pts
        lo += [l] * len(pts)
        hi += [h] * len(pts)
    return np.array(xs, dtype=f32), np.array(lo, dtype=f32), np.array(hi, dtype=f32)


def test_clamps_against_numpy_clip():
    """clampf / clamp01 = v_med3_f32 against np.clip for every non-NaN input: +-0, +-inf, denormals, x == lo, x == hi,
    lo == hi.  Bit-equal with +-0 identified.  (The NaN case is pinned in tests/test_hard_regime_gpu.py.)"""
    p = dp.probe("clamp", 256)
    x, lo, hi = clamp_arguments()
    r = p.points(x, c=lo, d=hi)
    bad = ~dp.same_value(r["out"][:, 0], dp.clamp(x, lo, hi))
    assert not bad.any(), (x[bad], lo[bad], hi[bad], r["out"][bad, 0])
    bad = ~dp.same_value(r["out"][:, 1], dp.clamp(x, 0.0, 1.0))
    assert not bad.any(), (x[bad], r["out"][bad, 1])
    # and a dense walk through the bounds of the kernels: [20, 20000], [0.1, 10], [0, 1]
    w = p.run(dp.bits(np.geomspace(1e-3, 1e5, 256).astype(f32)) | (np.arange(256) % 2 << 31), 8191,
              c=np.tile(f32([20.0, 0.1, 0.0, -0.7]), 64), d=np.tile(f32([20000.0, 10.0, 1.0, 0.7]), 64))
    bad = ~dp.same_value(w["out"][:, :, 0], dp.clamp(w["x"], w["c"][:, None], w["d"][:, None]))
    assert not bad.any(), (w["x"][bad][:8], w["out"][:, :, 0][bad][:8])
    bad = ~dp.same_value(w["out"][:, :, 1], dp.clamp(w["x"], 0.0, 1.0))
    assert not bad.any(), (w["x"][bad][:8], w["out"][:, :, 1][bad][:8])
    report("clampf / clamp01: arguments", len(x) + w["x"].size, error=False)
    report("clampf / clamp01: worst difference from np.clip", max(worst_difference(w["out"][:, :, 0], dp.clamp(w["x"], w["c"][:, None], w["d"][:, None])),
                                                                   worst_difference(r["out"][:, 0], dp.clamp(x, lo, hi))))


# ---------------------------------------------------------------------------------------------------------------------
# PolyBLEP
# ---------------------------------------------------------------------------------------------------------------------
BLEP_DT = (2.0e-7, 1.0e-4, 0.01, 0.2499, 1.0)
BLEP_DT_OFF = (0.0, 1.0e-45, 1.0e-8, float(dp.EPSILON))  # dt <= EPSILON: exactly 0, never NaN


def blep_arguments():
    """per dt: t from +0 and -0 through the denormals (both neighbours of 0), 64 floats either side of dt and of 1 - dt, 1 and
    its two neighbours, a dense run over [0, 1) and one over [0, dt).  Returns t bases, t strides, dt per voice."""
    a, sa, dt = [], [], []
    for v in BLEP_DT + BLEP_DT_OFF:
        v = f32(v)
        edges = np.array([v, f32(1.0) - v], dtype=f32)
        edges = edges[edges > dp.EPSILON]
        bases = np.concatenate([np.array([0x00000000, 0x80000000], dtype=np.uint64), dp.around(edges, 64), dp.around(f32(1.0), 254),
                                dp.bits(np.linspace(0.0, 1.0, 64, endpoint=False)).astype(np.uint64),
                                dp.bits(np.linspace(0.0, float(v), 16, endpoint=False)).astype(np.uint64)])
        strides = np.concatenate([np.ones(3 + len(edges)), np.full(64, 1021), np.full(16, 1021)])
        a.append(bases)
        sa.append(strides)
        dt.append(np.full(len(bases), v, dtype=f32))
    return np.concatenate(a), np.concatenate(sa).astype(np.uint64), np.concatenate(dt)


def test_polyblep_residuals_against_the_reference_with_true_division():
    """poly_blep / poly_blamp (rcp(dt) shared, one Newton step per quotient, both sides evaluated and selected) against
    oscillators/mod.rs:139-169 restated in numpy f32 with true division, for t over the phase's range [0, 1] and the
    neighbours of its ends.  Limits: blep 5e-7 (|dr/dx| <= 2 times 1 ulp(1) of the quotient, plus two roundings of values
    <= 2), blamp 2.5e-7 (|dr/dx| <= 1).  dt <= EPSILON returns exactly 0, never NaN."""
    a, sa, dt = blep_arguments()
    r = dp.probe("blep", 256).run(a, sa, dp.bits(dt), 0)
    t = r["x"]
    dtf = np.broadcast_to(dt[:, None], t.shape)
    assert np.array_equal(r["y"], dtf)
    inside = t <= np.nextafter(f32(1.0), f32(2.0))  # the phase and the float above 1; the walks around 1 - dt run further
    off = dtf <= dp.EPSILON
    for col, name, ref, limit in ((0, "poly_blep", dp.poly_blep(t, dtf), 5e-7), (1, "poly_blamp", dp.poly_blamp(t, dtf), 2.5e-7)):
        got = r["out"][:, :, col]
        assert (dp.bits(got[off]) & 0x7FFFFFFF == 0).all(), name
        assert (ref[off] == 0).all() and np.isfinite(got[inside]).all()
        for v in BLEP_DT:
            m = inside & (dtf == f32(v))
            assert (t[m] < dtf[m]).any() and (t[m] > f32(1.0) - dtf[m]).any() and (ref[m] != 0).any()
            err = float(np.max(np.abs(got[m].astype(np.float64) - ref[m])))
            report("%s, dt = %g: worst absolute error" % (name, v), err)
            assert err <= limit, (name, v, err)


# ---------------------------------------------------------------------------------------------------------------------
# the TPT coefficient forms
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tpt_sweep(sr):
    """(h, g, k) of the three forms over the cases of one sample rate: {"cutoff", "q", "layout": per lane, "out": [form]}"""
    s = dp.tpt_slots(sr)
    lanes, layout = dp.tpt_layout(dp.tpt_cutoffs(sr), s)
    assert len(lanes) % 64 == 0
    cutoff = np.tile(lanes, len(dp.TPT_QS))
    q = np.repeat(f32(dp.TPT_QS), len(lanes))
    p = dp.probe("tpt", 4096)
    assert p.eng.lanes_per_voice == 1 and p.eng.voices_per_wave >= 2
    out = []
    for form in (0, 1, 2):
        r = p.points(cutoff, c=q, sel=form, u0=s["two_sr"], u1=s["period"], u2=s["nyquist"], u3=s["max_cutoff"])
        assert (r["out"][:, 3] == form).all()
        out.append(r["out"][:, :3])
    return {"cutoff": cutoff, "q": q, "layout": np.tile(layout, len(dp.TPT_QS)), "out": out, "slots": s}


@pytest.mark.parametrize("sr", dp.TPT_RATES)
def test_tpt_coefficient_forms_agree_and_follow_the_f64_formula(sr):
    """tpt_update_coefficients, tpt_update_coefficients_iq (inv_q = 1.0f / q) and tpt_params_nomod_flat (from sentinel
    cur_c / cur_q) over a geometric run of cutoffs from 20 Hz to max_cutoff, the floats either side of the cutoff where the
    tangent's argument x crosses pi/4 and the 64 floats below max_cutoff, at q 0.1 / 0.707 / 10; the lanes in waves wholly
    below pi/4, wholly above, and with odd lanes above and even lanes below (the wave-uniform __any of the _iq form).
    (a) _iq == tpt_update_coefficients bit for bit in every layout; (b) the flat form == both bit for bit where x <= pi/4,
    above it g within 1 ulp with h and k following; (c) all three against the f64 formula on the f32 x: g to 2.5e-7 (the
    bound tests/test_og_math.py holds for og_tanf_q1) + 2.4e-7 relative, k to the same absolute error plus one rounding, h to
    2 rel(g) + 3 ulp; (d) at Nyquist for sample rates up to 40 kHz the sign of g is the sign of libm's tanf(x)."""
    w = tpt_sweep(sr)
    s, cutoff, q, layout = w["slots"], w["cutoff"], w["q"], w["layout"]
    std, iq, flat = w["out"]
    x = dp.tpt_x(cutoff, s)
    above = x > dp.PIO4
    for code in (0, 1, 2):  # the three layouts are there, block by block
        blocks = above[layout == code].reshape(-1, 64)
        assert len(blocks) >= 3
        if code == 0:
            assert not blocks.any()
        elif code == 1:
            assert blocks.all()
        else:
            assert blocks[:, 1::2].all() and not blocks[:, 0::2].any()
    # (a)
    assert np.array_equal(dp.bits(iq), dp.bits(std)), np.argwhere(dp.bits(iq) != dp.bits(std))[:8]
    # (b)
    assert np.array_equal(dp.bits(flat[~above]), dp.bits(std[~above]))
    dg = dp.ulp_distance(flat[:, 1], std[:, 1])
    report("flat form above pi/4, %g Hz: worst distance of g in ulp" % sr, dg[above].max(), error=False)
    report("flat form above pi/4, %g Hz: share of g that differs" % sr, float(np.mean(dg[above] != 0)), error=False)
    assert dg.max() <= 1
    inv_q = (f32(1.0) / q).astype(f32)
    assert np.array_equal(dp.bits(flat[:, 2]), dp.bits((flat[:, 1] + inv_q).astype(f32)))  # k = f + inv_q of ITS g
    same = dg == 0
    assert np.array_equal(dp.bits(flat[same]), dp.bits(std[same]))
    # h = 1 / (1 + f/q + f^2): |dh/h| <= 2 |df/f|, and 1 ulp of g is at most 1.19e-7 relative; one rounding on each side
    hs, hf = std[:, 0].astype(np.float64), flat[:, 0].astype(np.float64)
    assert (np.abs(hf - hs) <= 2 * 1.1920929e-7 * hs + 2 * np.spacing(std[:, 0])).all()
    # (c)
    h_ref, g_ref, k_ref = dp.tpt_reference(cutoff, q, s)
    g_lim = 2.5e-7 + 2.4e-7
    for name, got in (("tpt_update_coefficients", std), ("tpt_update_coefficients_iq", iq), ("tpt_params_nomod_flat", flat)):
        h, g, k = (got[:, i].astype(np.float64) for i in range(3))
        rel_g = np.abs(g - g_ref) / np.abs(g_ref)
        err_k = np.abs(k - k_ref) - (g_lim * np.abs(g_ref) + 0.5 * np.spacing(np.abs(k_ref).astype(f32)))
        rel_h = np.abs(h - h_ref) / h_ref - 3 * np.spacing(got[:, 0]) / h_ref
        report("%s, %g Hz: worst relative error of g" % (name, sr), rel_g.max())
        report("%s, %g Hz: worst relative error of h" % (name, sr), (np.abs(h - h_ref) / h_ref).max())
        assert rel_g.max() <= g_lim, (name, cutoff[np.argmax(rel_g)], rel_g.max())
        assert err_k.max() <= 0, (name, cutoff[np.argmax(err_k)])
        assert (rel_h <= 2 * g_lim).all(), (name, cutoff[np.argmax(rel_h)], rel_h.max())
    # (d)
    if sr <= 40000.0:
        top = cutoff == s["max_cutoff"]
        assert s["max_cutoff"] == s["nyquist"] and top.sum() >= 6
        sign = np.sign(dp.host_libm("tanf", x[top]))
        report("tan at Nyquist, %g Hz: g" % sr, float(std[top, 1][0]), error=False)
        for got in (std, iq, flat):
            assert np.array_equal(np.sign(got[top, 1]), sign)
        if sr in (32000.0, 8000.0):
            assert (sign < 0).all()
