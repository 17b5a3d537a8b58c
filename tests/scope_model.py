"""A numpy float32 restatement of the reference's Oscilloscope (oscen-lib/src/oscilloscope/mod.rs), one object per voice: the
witness of tests/test_oscilloscope_gpu.py.  Line numbers are those of mod.rs.

One deliberate difference.  store_triggered (111-123) and snapshot (67-109) index the ring with
`counter.wrapping_sub(1 + offset).rem_euclid(capacity)`.  While fewer than `length` samples have been pushed the subtraction
wraps around usize, and (2^64 - k) mod capacity equals (-k) mod capacity only for a capacity that is a power of two: there the
reference reads slots nobody has written yet, which hold 0.0; for any other capacity it lands on a slot that depends on the
width of usize (2^64 mod 7 = 2, 2^32 mod 7 = 4).  Here, as on the device, the samples in front of the first push are 0.0 for
every capacity.  (snapshot never reaches below the first push: it hands out at most `written` samples.)"""
import numpy as np

f32 = np.float32


class Scope:
    def __init__(self, capacity, auto_detect=False):
        self.capacity = max(int(capacity), 1)            # :21
        self.ring = np.zeros(self.capacity, dtype=f32)   # :23
        self.counter = 0                                 # :24
        self.written = 0                                 # :25
        self.triggered = np.zeros(self.capacity, dtype=f32)  # :27
        self.triggered_length = 0                        # :28
        self.trigger_period = f32(self.capacity)         # :186, 201, 216
        self.trigger_enabled = f32(1.0)                  # :187
        self.last_sample = f32(0.0)
        self.auto_detect = bool(auto_detect)             # :189, 204, 219
        self.period_sample_count = 0
        self.detected_period = self.capacity             # :191

    def push(self, x):                                   # :51-65
        self.ring[self.counter % self.capacity] = x
        self.counter += 1
        self.written = min(self.written + 1, self.capacity)

    def last(self, n):
        """the last n pushed samples in time order; what lies in front of the first push is 0.0 (see the module text)"""
        t = self.counter - n + np.arange(n)
        return np.where(t >= 0, self.ring[t % self.capacity], f32(0.0)).astype(f32)

    def store_triggered(self, length):                   # :111-123
        length = max(min(length, self.capacity), 1)
        self.triggered[:length] = self.last(length)
        self.triggered_length = length

    def clear_triggered(self):                           # :125-127
        self.triggered_length = 0

    def snapshot(self, sample_count):                    # :67-109
        available = min(self.written, self.capacity)
        if available == 0:
            return np.zeros(0, f32), np.zeros(0, f32)
        requested = min(max(int(sample_count), 1), available)
        n = min(self.triggered_length, self.capacity)
        return self.last(requested), self.triggered[:n].copy()

    def process(self, x, trigger_period=None, trigger_enabled=None):  # :241-286
        x = f32(x)
        if trigger_period is not None:
            self.trigger_period = f32(trigger_period)
        if trigger_enabled is not None:
            self.trigger_enabled = f32(trigger_enabled)
        self.push(x)
        if self.trigger_enabled > f32(0.5):              # :249 (false for a NaN)
            crossing = bool(self.last_sample <= f32(0.0) and x > f32(0.0))  # :251
            if self.auto_detect:
                self.period_sample_count += 1            # :255
                if crossing:
                    if self.period_sample_count > 1:     # :259-263
                        self.detected_period = max(min(self.period_sample_count, self.capacity), 10)
                    if self.detected_period > 0:         # :266-268
                        self.store_triggered(self.detected_period)
                    self.period_sample_count = 0         # :271
            elif crossing:                               # :275-281
                p = self.trigger_period
                p = f32(1.0) if not (p > f32(1.0)) else p   # f32::max(NaN, 1.0) = 1.0
                # f32::round: half away from zero (p >= 1: floor(p + 0.5), exact in float64); `as usize` saturates
                length = self.capacity if p >= f32(self.capacity) else int(np.floor(np.float64(p) + 0.5))
                if length > 0:
                    self.store_triggered(length)
        self.last_sample = x                             # :285
        return x                                         # :246


def run(x, capacity, auto_detect=False, trigger_period=None, trigger_enabled=None, scopes=None):
    """x[voice][frame] through one Scope per voice.  trigger_period / trigger_enabled: None (the defaults), a scalar, [voice] or
    [voice][frame].  scopes: continue these.  Returns the scopes."""
    x = np.asarray(x, dtype=f32)
    n, frames = x.shape
    if scopes is None:
        scopes = [Scope(capacity, auto_detect) for _ in range(n)]

    def per(a, v, f):
        if a is None:
            return None
        a = np.asarray(a, dtype=f32)
        return a if a.ndim == 0 else (a[v] if a.ndim == 1 else a[v, f])

    for v in range(n):
        s = scopes[v]
        for f in range(frames):
            s.process(x[v, f], per(trigger_period, v, f), per(trigger_enabled, v, f))
    return scopes


def known_answers():
    """the reference's own three tests (mod.rs:293-323) on this model"""
    h = Scope(8)
    for i in range(10):
        h.push(f32(i))
    s, t = h.snapshot(4)
    assert np.array_equal(s, np.array([6, 7, 8, 9], f32)) and t.size == 0
    h = Scope(16)
    s, t = h.snapshot(8)
    assert s.size == 0 and t.size == 0
    h = Scope(4)
    for i in range(4):
        h.push(f32(i))
    s, t = h.snapshot(16)
    assert np.array_equal(s, np.array([0, 1, 2, 3], f32)) and t.size == 0
    return True
