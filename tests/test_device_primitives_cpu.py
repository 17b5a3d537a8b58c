"""The witnesses of tests/test_device_primitives_gpu.py, checked on the CPU: the numpy references against hand-worked values,
the host build of the tangent forms against libm over the TPT cases, and that the argument walks contain the edge sets the
GPU assertions call non-empty.  No GPU, no sanitizer."""
import numpy as np

from tests import device_probe as dp
from tests import test_device_primitives_gpu as gpu

f32 = np.float32
BELOW_ONE = f32(0.99999994)


def sign_bit(x):
    return dp.bits(x) >> 31


def test_fract_references_on_hand_worked_values():
    x = f32([0.25, -0.25, 2.5, -2.5, 3.0, -3.0, 0.0, -0.0, 2.0 ** 24 + 2, -(2.0 ** 23) - 1])
    assert np.array_equal(dp.rem_euclid1(x), f32([0.25, 0.75, 0.5, 0.5, 0, 0, 0, 0, 0, 0]))
    assert np.array_equal(dp.fmod1(x), f32([0.25, -0.25, 0.5, -0.5, 0, 0, 0, 0, 0, 0]))
    assert not sign_bit(dp.fmod1(f32([-3.0, -0.0]))).any()  # x - trunc(x) is +0 for a negative whole x and for -0
    # 1 + x for a small negative x: halfway between 1 - 2^-24 and 1.0 at x = -2^-25, and the tie goes to even
    tie = f32(-2.0 ** -25)
    assert tie == gpu.TIE
    near = f32([tie, np.nextafter(tie, f32(-1)), np.nextafter(tie, f32(0)), -2.0 ** -24, -1.0e-45, -6.0e-8, -3.0e-8, -2.9e-8])
    assert np.array_equal(dp.rem_euclid1(near), f32([1.0, BELOW_ONE, 1.0, BELOW_ONE, 1.0, BELOW_ONE, BELOW_ONE, 1.0]))
    assert dp.bits(BELOW_ONE)[0] == 0x3F7FFFFF
    assert np.array_equal(dp.rem_euclid1(f32([-0.75, -1.0e-3])), f32([0.25, f32(1.0) + f32(-1.0e-3)]))


def test_clamp_reference_on_hand_worked_values():
    inf = np.inf
    x = f32([0.5, -0.5, 2.0, 0.0, -0.0, inf, -inf, 1.0e-45, 20.0, 20000.0, 5.0, 4.0, 6.0])
    lo = f32([0, 0, 0, 0, 0, 0, 0, 0, 20, 20, 5, 5, 5])
    hi = f32([1, 1, 1, 1, 1, 1, 1, 1, 20000, 20000, 5, 5, 5])
    want = f32([0.5, 0, 1, 0, 0, 1, 0, 1.0e-45, 20, 20000, 5, 5, 5])
    assert np.array_equal(dp.clamp(x, lo, hi), want)
    assert dp.same_value(f32([0.0]), f32([-0.0])).all() and not dp.same_value(f32([0.0]), f32([1.0e-45])).any()
    assert dp.ulp_distance(f32([1.0e-45, 1.0]), f32([-1.0e-45, np.nextafter(f32(1), f32(2))])).tolist() == [2, 1]


def test_polyblep_references_on_hand_worked_values():
    # mod.rs:139-169: t < dt: x = t / dt, 2x - x^2 - 1;  t > 1 - dt: x = (t - 1) / dt, x^2 + 2x + 1;  blamp: -(x - 1)^3 / 3, (x + 1)^3 / 3
    assert np.array_equal(dp.poly_blep(f32([0.0, 0.125, 0.5, 0.875]), f32(0.25)), f32([-1.0, -0.25, 0.0, 0.25]))
    assert np.array_equal(dp.poly_blamp(f32([0.0, 0.5]), f32(0.25)), f32([f32(1) / f32(3), 0.0]))
    assert np.array_equal(dp.poly_blamp(f32([0.875]), f32(0.25)), f32([f32(0.125) / f32(3)]))
    off = f32(gpu.BLEP_DT_OFF)
    assert (off <= dp.EPSILON).all() and off[-1] == dp.EPSILON
    for t in f32([0.0, 1.0e-45, 0.5, 1.0]):
        assert (dp.poly_blep(np.full(4, t), off) == 0).all() and (dp.poly_blamp(np.full(4, t), off) == 0).all()


def test_walks_are_consecutive_bit_patterns():
    w = dp.walk(dp.around(f32([1.0, -1.0]), 2), 1, frames=5)
    assert np.array_equal(w[0], f32([1 - 2.0 ** -23, 1 - 2.0 ** -24, 1, 1 + 2.0 ** -23, 1 + 2.0 ** -22]))
    assert np.array_equal(w[1], -w[0])
    assert np.array_equal(dp.bits(dp.walk([0xFFFFFFFF], 3, frames=2, tick0=1)), [[2, 5]])  # modulo 2^32, as the lanes add


def test_host_build_of_the_tangent_forms_against_libm_over_the_tpt_cases():
    """og_tanf_q1 as the three coefficient forms call it, at the arguments the cases form: 2.5e-7 relative (the bound of
    tests/test_og_math.py) also on the last floats below pi/2, where the tangent is +-6e6 .. 1.3e7; same sign as libm; negative
    at Nyquist for 32 000 and 8 000 Hz, where the f32 products land x one float above fl(pi/2), beyond pi/2."""
    for sr in dp.TPT_RATES:
        s = dp.tpt_slots(sr)
        cut = dp.tpt_cutoffs(sr)
        x = dp.tpt_x(cut, s)
        assert cut[0] == 20.0 and cut[-1] == s["max_cutoff"] and len(cut) >= 160 + 64
        assert (x <= dp.PIO4).any() and (x > dp.PIO4).any()
        edge = np.flatnonzero(x > dp.PIO4)[0]  # the floats either side of the crossing are there
        assert dp.ulp_distance(cut[edge], cut[edge - 1]) == 1 and dp.ulp_distance(cut[edge + 1], cut[edge - 2]) == 3
        assert (np.diff(dp.ordered(cut[-65:])) == 1).all()
        got, ref = dp.host_eval("tangent", x)[:, 1].astype(np.float64), dp.host_libm("tanf", x).astype(np.float64)
        assert np.max(np.abs(got - ref) / np.abs(ref)) <= 2.5e-7
        assert np.array_equal(np.sign(got), np.sign(ref))
        if sr <= 40000.0:
            assert s["max_cutoff"] == s["nyquist"] == f32(sr / 2) and abs(got[-1]) > 6e6
            assert dp.ulp_distance(x[-1], f32(np.pi / 2)) <= 1
        if sr in (32000.0, 8000.0):
            assert float(x[-1]) > np.pi / 2 and got[-1] < 0 and ref[-1] < 0
        h, g, k = dp.tpt_reference(cut[:1], f32(0.70710678), s)  # 20 Hz: g = tan(pi 20 / sr) to first order
        assert abs(g[0] / (np.pi * 20.0 / sr) - 1) < 1e-3 and abs(k[0] - g[0] - 2 ** 0.5) < 1e-6 and 0 < h[0] < 1


def test_tpt_layouts_hold_whole_low_whole_high_and_mixed_waves():
    for sr in dp.TPT_RATES:
        s = dp.tpt_slots(sr)
        cut = dp.tpt_cutoffs(sr)
        lanes, layout = dp.tpt_layout(cut, s)
        above = dp.tpt_x(lanes, s) > dp.PIO4
        assert len(lanes) % 64 == 0 and len(lanes) * len(dp.TPT_QS) <= 4096
        assert not above[layout == 0].any() and above[layout == 1].all()
        mixed = above[layout == 2].reshape(-1, 64)
        assert len(mixed) >= 1 and mixed[:, 1::2].all() and not mixed[:, 0::2].any()
        for code in (0, 1, 2):
            assert np.flatnonzero(layout == code)[0] % 64 == 0
        for part in (lanes[layout < 2], lanes[layout == 2]):  # every case sits in a uniform wave AND in a mixed one
            assert np.array_equal(np.unique(part), cut)


def test_argument_walks_contain_the_edge_sets():
    # fract: the arguments where the reference gives 1.0, the tie itself, negative whole numbers, -0, +-(2^23 - 2 .. 2^24 + 2)
    a, sa, where = gpu.concat_sets(gpu.fract_arguments())
    x = dp.walk(a, sa)
    assert ((x >= gpu.TIE) & (x < 0)).sum() > 60000 and (x == gpu.TIE).any() and (x == np.nextafter(gpu.TIE, f32(-1))).any()
    neg_whole = np.signbit(x) & (x == np.trunc(x))
    assert (neg_whole & (np.abs(x) < 2.0 ** 23) & (x != 0)).sum() >= 1023 and (dp.bits(x) == 0x80000000).any()
    big = np.abs(x[where["big"]])
    assert big.min() == 2.0 ** 23 - 2 and big.max() == 2.0 ** 24 + 2 and (x[where["big"]] < 0).any()
    assert (np.abs(x[where["dense"]]) <= 4.6).all() and (x == 0).any()
    assert ((x != 0) & (np.abs(x) < 1.2e-38)).sum() > 1000  # denormals of both signs
    a, chunk = gpu.fract_every_float()  # chunk after chunk from the smallest negative denormal to -2^-23, nothing left out
    e = dp.bits(dp.walk(a, chunk)).astype(np.int64).ravel()
    assert (np.diff(e) == chunk).all() and e[0] == 0x80000001 and dp.from_bits([e[-1] + chunk - 1])[0] == f32(-2.0 ** -23)
    # exact sine / cosine: a million arguments below 120, the named floats and 64 neighbours either side
    bulk, edge = gpu.exact_arguments()
    a, sa, _ = gpu.concat_sets(bulk)
    x = dp.walk(a, sa)
    assert (np.abs(x) < 120).all() and x.size >= 1000000 and np.abs(x).min() < 2.0 ** -12 and np.abs(x).max() > 119.9
    a, sa, _ = gpu.concat_sets(edge)
    e = dp.walk(a, sa, frames=129)
    for c in [np.pi / 4, 2.0 ** -12, 120.0] + [k * np.pi / 2 for k in range(1, 77)]:
        for sgn in (1.0, -1.0):
            row = e[np.flatnonzero(e[:, 64] == f32(sgn * c))[0]]
            assert (np.diff(dp.ordered(np.abs(row))) == 1).all()
    assert (dp.bits(e[:, 0]) == 0).any() and (dp.bits(e[:, 0]) == 0x80000000).any()
    # sines: the exact quarter turns, +-16 turns, [-1, 2)
    a, sa, where = gpu.concat_sets(gpu.sine_arguments())
    x = dp.walk(a, sa)
    assert np.array_equal(np.sort(x[where["quarters"]][:, 128] * 4), np.setdiff1d(np.arange(-64, 65), [0]))
    assert -1.01 < x[where["unit"]].min() <= -1.0 and 1.99 < x[where["unit"]].max() < 2.0
    assert np.abs(x[where["turns16"]]).max() >= 16 and np.abs(x[where["pm1e5"]]).max() >= 1e5
    # quotients: the documented domain from 1 to 2^40 with every magnitude of a, PolyBLEP's from EPSILON to 1
    args = gpu.divide_arguments()
    b = np.concatenate([dp.walk(args[k]["b"], args[k]["sb"]).ravel() for k in ("documented", "documented_top")])
    assert b.min() == 1.0 and b.max() == 2.0 ** 40
    b, t = dp.walk(args["blep"]["b"], args["blep"]["sb"]), dp.walk(args["blep"]["a"], args["blep"]["sa"])
    assert b.min() == np.nextafter(dp.EPSILON, f32(1)) and 0.99 < b.max() <= 1.0 and np.abs(t).max() <= 1.0 and (t < 0).any()
    den = gpu.tpt_denominators()
    assert den.min() >= 1.0 and den.max() > 1e13 and len(den) >= 15 * 224
    # PolyBLEP: per dt both selected sides and the neighbours of 0 and 1
    a, sa, dt = gpu.blep_arguments()
    t = dp.walk(a, sa)
    for v in gpu.BLEP_DT:
        m = t[dt == f32(v)]
        for c in (0.0, 1.0):
            assert (m == f32(c)).any() and (m == np.nextafter(f32(c), f32(2))).any() and (m == np.nextafter(f32(c), f32(-1))).any()
        for c in (f32(v), f32(1.0) - f32(v)):
            assert (m == c).any() and (m == np.nextafter(c, f32(2))).any() and (m == np.nextafter(c, f32(-1))).any()
    # clamps
    x, lo, hi = gpu.clamp_arguments()
    assert (x == lo).any() and (x == hi).any() and (lo == hi).any() and np.isinf(x).any() and not np.isnan(x).any()
    assert (dp.bits(x) == 0x80000000).any() and ((x != 0) & (np.abs(x) < 1e-38)).any() and (lo <= hi).all()
