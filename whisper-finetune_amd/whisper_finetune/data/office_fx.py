"""Office effects: the draws of the bit-crush and room-reverb augmentation (pure Python / numpy; the sibling of filters.py, wave_fx.py
and rate_fx.py).

The reference's office pipeline (`get_audio_augments_office`, model/augment.py) is a Compose of two groups:

  OneOf([Mp3Compression, BitCrush(min_bit_depth=6, max_bit_depth=14)], p=0.5)
  OneOf([RoomSimulator(shoebox, absorption 0.05-0.20, max_order=3, leave_length_unchanged=True)], p=0.5)

BitCrush and the room simulation run on the device (csrc/office.hip, include/wft.h "Office effects" states the arithmetic): the bit
crush is three f32 operations per sample, the room a shoebox impulse response designed HERE, in a loader worker, and convolved over
the clip by `wft_fir_conv_f32`.  This module designs the response (`room_ir`) and draws a clip's parameters (`OfficeAug`); a worker
ships them as one table row f64 [2 + cap]: the bit depth (0 = no crush), n_taps (0 = no room), then the response, zero behind n_taps.

Deviations from the reference's recipe, all of them deliberate:
  * the image-source method only.  audiomentations' default use_ray_tracing=True is stochastic inside pyroomacoustics and is not
    restated, so there is no late tail beyond max_order.
  * no air absorption, no output normalisation.
  * Mp3Compression needs a codec and is not built: its slot in the first group is dropped.
  * own gates that reproduce the reference's MARGINAL rates: crush 0.5 * 1/2 = 0.25, room 0.5.
  * pyroomacoustics and audiomentations are not dependencies: the method is restated from its definition, parity with their binaries
    is unpinned.
  * timestamps are untouched, as in the reference.
"""
from __future__ import annotations

import math
import random
from typing import Mapping

import numpy as np

SOUND_SPEED = 343.0     # m/s
FDL = 81                # taps of the fractional-delay filter
FDL2 = FDL // 2
BLOCK = 1024            # wft_fir_conv_f32's block: the table's response is padded to a multiple of it
TAPS_MAX = 8192         # wft_fir_conv_f32's limit
BITS_MAX = 24           # wft_bitcrush_f32's limit: 2^24 + 1 is not an f32
WALL_MARGIN = 0.1       # m: source and microphone stay this far inside the room
STAGES = ("crush", "room")
DEFAULT_P = {"crush": 0.5 / 2.0, "room": 0.5}
ROOM_DEFAULTS = dict(min_size_x=3.0, max_size_x=5.0, min_size_y=2.5, max_size_y=4.0, min_size_z=2.4, max_size_z=3.0,
                     min_absorption_value=0.05, max_absorption_value=0.20,
                     min_source_x=0.1, max_source_x=3.5, min_source_y=0.1, max_source_y=2.7, min_source_z=1.0, max_source_z=2.1,
                     min_mic_distance=0.15, max_mic_distance=0.35, max_order=3)


def _hann(n: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / (n - 1))  # np.hanning: symmetric


def image_sources(size, source, max_order: int):
    """The images of `source` in the shoebox [0, size] with at most max_order reflections in total: (positions f64 [M, 3],
    reflections i64 [M]).  Along an axis of length L the image of index a lies at a * L + s for an even a and at (a + 1) * L - s for
    an odd one, after |a| reflections; every triple with |a| + |b| + |c| <= max_order counts (7 at order 1, 63 at order 3)."""
    size, source = np.asarray(size, dtype=np.float64), np.asarray(source, dtype=np.float64)
    pos, refl = [], []
    r = range(-max_order, max_order + 1)
    for a in r:
        for b in r:
            for c in r:
                order = abs(a) + abs(b) + abs(c)
                if order > max_order:
                    continue
                idx = np.array([a, b, c])
                pos.append(np.where(idx % 2 == 0, idx * size + source, (idx + 1) * size - source))
                refl.append(order)
    return np.array(pos, dtype=np.float64), np.array(refl, dtype=np.int64)


def room_ir(size, source, mic, absorption: float, max_order: int = 3, sample_rate: int = 16000) -> np.ndarray:
    """The impulse response from `source` to `mic` in the shoebox room of `size` (x, y, z in metres) whose walls all absorb the share
    `absorption` of the energy: the image-source method as pyroomacoustics defines it, restated.  Every image with at most max_order
    reflections in total contributes (1 - absorption)^(r / 2) / (4 pi d) for r reflections at distance d, delayed by d * fs / c
    samples (c = 343 m/s) and placed with an 81-tap Hann-windowed sinc fractional delay: with i = floor(delay), the taps
    hann[k] * sinc(k - 40 - (delay - i)) go to ir[i + k], k < 81 (so the sample of delay 0 sits at index 40).  The length is
    floor(max delay) + 81.  Computed in float64, returned as float32.  A bad argument raises ValueError."""
    size, source, mic = (np.asarray(v, dtype=np.float64) for v in (size, source, mic))
    if size.shape != (3,) or source.shape != (3,) or mic.shape != (3,) or not np.all(np.isfinite(np.concatenate([size, source, mic]))):
        raise ValueError("room_ir: size, source and mic must be three finite numbers each")
    if not np.all(size > 0) or not (np.all(source >= 0) and np.all(source <= size) and np.all(mic >= 0) and np.all(mic <= size)):
        raise ValueError(f"room_ir: source {source.tolist()} and mic {mic.tolist()} must lie inside the room {size.tolist()}")
    if isinstance(absorption, bool) or not isinstance(absorption, (int, float)) or not 0.0 <= absorption <= 1.0:
        raise ValueError(f"room_ir: absorption must lie in [0, 1], got {absorption!r}")
    if isinstance(max_order, bool) or not isinstance(max_order, int) or not 0 <= max_order <= 16:
        raise ValueError(f"room_ir: max_order must be an integer inside [0, 16], got {max_order!r}")
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate < 1:
        raise ValueError(f"room_ir: sample_rate must be a positive integer, got {sample_rate!r}")
    pos, refl = image_sources(size, source, max_order)
    dist = np.sqrt(((pos - mic) ** 2).sum(axis=1))
    if not np.all(dist > 0):
        raise ValueError("room_ir: source and mic coincide")
    amp = (1.0 - float(absorption)) ** (refl / 2.0) / (4.0 * np.pi * dist)
    delay = dist * float(sample_rate) / SOUND_SPEED
    whole = np.floor(delay)
    ir = np.zeros(int(whole.max()) + FDL, dtype=np.float64)
    window, k = _hann(FDL), np.arange(FDL, dtype=np.float64) - FDL2
    for a, i, frac in zip(amp, whole.astype(np.int64), delay - whole):
        ir[i:i + FDL] += a * window * np.sinc(k - frac)
    return ir.astype(np.float32)


def table_cap(max_size, max_order: int, sample_rate: int = 16000) -> int:
    """The response length a table row reserves: the smallest multiple of 1024 that is >= fs * (max_order + 1) * diag_max / c + 81
    (an image of r reflections lies at most (r + 1) room diagonals away) — 2048 at the defaults."""
    diag = math.sqrt(sum(float(v) ** 2 for v in max_size))
    need = float(sample_rate) * (max_order + 1) * diag / SOUND_SPEED + FDL
    return int(math.ceil(need / BLOCK)) * BLOCK


def none_table(cap: int, B=None) -> np.ndarray:
    """The table of "neither stage": f64 [2 + cap], or [B, 2 + cap]."""
    return np.zeros(2 + cap if B is None else (B, 2 + cap), dtype=np.float64)


def check_table(table) -> np.ndarray:
    """f64 [B, 2 + cap] (a tensor or an array) -> the same as a float64 numpy array, checked: cap a multiple of 1024 inside
    [1024, 8192]; the bit depth an integer, 0 or inside [1, 24]; n_taps an integer inside [0, cap]; the response finite, fit for
    float32 and zero behind n_taps.  ValueError otherwise."""
    t = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table)
    if t.dtype != np.float64 or t.ndim != 2 or t.shape[1] < 2 + BLOCK or (t.shape[1] - 2) % BLOCK or t.shape[1] - 2 > TAPS_MAX:
        raise ValueError(f"office_fx table must be float64 [B, 2 + cap] with cap a multiple of {BLOCK} up to {TAPS_MAX}, got {t.dtype} {tuple(t.shape)}")
    cap = t.shape[1] - 2
    bits, taps, ir = t[:, 0], t[:, 1], t[:, 2:]
    if not bool(np.all((bits == np.rint(bits)) & (bits >= 0) & (bits <= BITS_MAX))):  # (NaN fails)
        raise ValueError(f"office_fx table: the bit depth must be an integer inside [1, {BITS_MAX}], or 0")
    if not bool(np.all((taps == np.rint(taps)) & (taps >= 0) & (taps <= cap))):
        raise ValueError(f"office_fx table: n_taps must be an integer inside [0, {cap}]")
    if not bool(np.all(np.isfinite(ir)) and np.all(np.abs(ir) <= float(np.finfo(np.float32).max))):
        raise ValueError("office_fx table: the response must be finite float32 values")
    if bool(np.any((np.arange(cap)[None, :] >= taps[:, None]) & (ir != 0))):
        raise ValueError("office_fx table: the response must be zero behind n_taps")
    return np.ascontiguousarray(t)


def _group(spec, name: str, keys):
    if not isinstance(spec, Mapping) or not set(spec.keys()) <= set(keys):
        raise ValueError(f"OfficeAug {name} must be None or a mapping with the keys {sorted(keys)}, got {spec!r}")
    p = spec.get("p", DEFAULT_P[name])
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"OfficeAug {name}: p must lie in [0, 1], got {p!r}")
    return float(p)


def _pair(spec, lo: str, hi: str, defaults, low: float, high: float):
    a, b = spec.get(lo, defaults[lo]), spec.get(hi, defaults[hi])
    if any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in (a, b)) or not (math.isfinite(a) and math.isfinite(b) and a <= b):
        raise ValueError(f"OfficeAug: need finite numbers {lo} <= {hi}, got {a!r}, {b!r}")
    if a < low or b > high:
        raise ValueError(f"OfficeAug: {lo}..{hi} must stay inside [{low}, {high}], got {a!r}, {b!r}")
    return float(a), float(b)


class OfficeAug:
    """OfficeAug(sample_rate, crush=None | {p, min_bit_depth, max_bit_depth}, room=None | {p, min/max_size_x/y/z,
    min/max_absorption_value, min/max_source_x/y/z, min/max_mic_distance, max_order}); a missing group is off, `{}` = the defaults:
    p = DEFAULT_P (the reference's marginal rates 0.25 and 0.5), the reference's call (bit depth 6-14, room 3-5 x 2.5-4 x 2.4-3 m,
    absorption 0.05-0.20, max_order 3) and audiomentations' RoomSimulator defaults for what the reference leaves unset (source x
    0.1-3.5, y 0.1-2.7, z 1.0-2.1, microphone 0.15-0.35 m from the source).

    draw() -> (names, row): names = {"crush": bool, "room": bool}, row = the clip's table row f64 [2 + cap] (module docstring);
    cap = table_cap(largest room, max_order), 2048 at the defaults; a max_order whose cap exceeds 8192 raises ValueError.  All draws
    use Python's `random` module and never touch torch's generator; a dataset makes them AFTER the rate-effects draw, so every stream
    of draws that existed before is unchanged.  For each group that is on, in the order crush, room:
      1. the gate:  random.random() < p; if it fails nothing else is drawn for the group
      2. crush:     random.randint(min_bit_depth, max_bit_depth)
         room:      size x, y, z; the absorption; source x, y, z; the microphone's distance, azimuth in [0, 2 pi) and elevation in
                    [-pi/2, pi/2] — ten random.uniform calls in that order.  Source and microphone are clamped to 0.1 m inside the
                    room; a microphone that the clamps put onto the source is moved 0.15 m along x (towards the room's middle).
    Every range is checked in the constructor (ValueError)."""

    def __init__(self, sample_rate: int = 16000, crush=None, room=None):
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate < 1000:
            raise ValueError(f"OfficeAug sample_rate must be an integer >= 1000, got {sample_rate!r}")
        self.sample_rate = sample_rate
        self.p, self.bit_range, self.room = {}, None, None
        self.cap = BLOCK
        if crush is not None:
            self.p["crush"] = _group(crush, "crush", ("p", "min_bit_depth", "max_bit_depth"))
            lo, hi = _pair(crush, "min_bit_depth", "max_bit_depth", dict(min_bit_depth=6, max_bit_depth=14), 1, BITS_MAX)
            if lo != int(lo) or hi != int(hi):
                raise ValueError(f"OfficeAug crush: bit depths must be integers, got {lo!r}, {hi!r}")
            self.bit_range = (int(lo), int(hi))
        if room is not None:
            self.p["room"] = _group(room, "room", ("p",) + tuple(ROOM_DEFAULTS))
            order = room.get("max_order", ROOM_DEFAULTS["max_order"])
            if isinstance(order, bool) or not isinstance(order, int) or not 0 <= order <= 16:
                raise ValueError(f"OfficeAug room: max_order must be an integer inside [0, 16], got {order!r}")
            r = {"max_order": order}
            for axis in "xyz":
                r["size_" + axis] = _pair(room, f"min_size_{axis}", f"max_size_{axis}", ROOM_DEFAULTS, 4 * WALL_MARGIN, 100.0)
                r["source_" + axis] = _pair(room, f"min_source_{axis}", f"max_source_{axis}", ROOM_DEFAULTS, 0.0, 100.0)
            r["absorption"] = _pair(room, "min_absorption_value", "max_absorption_value", ROOM_DEFAULTS, 0.0, 1.0)
            r["mic_distance"] = _pair(room, "min_mic_distance", "max_mic_distance", ROOM_DEFAULTS, 0.01, 100.0)
            self.room = r
            self.cap = table_cap([r["size_" + axis][1] for axis in "xyz"], order, sample_rate)
            if self.cap > TAPS_MAX:
                raise ValueError(f"OfficeAug room: max_order {order} in rooms up to {[r['size_' + a][1] for a in 'xyz']} m needs responses "
                                 f"of up to {self.cap} taps, more than the {TAPS_MAX} of wft_fir_conv_f32")

    def draw_room(self):
        """The room group's ten draws -> (size, source, mic, absorption), clamped as the class docstring says."""
        r = self.room
        size = np.array([random.uniform(*r["size_" + a]) for a in "xyz"])
        absorption = random.uniform(*r["absorption"])
        source = np.array([random.uniform(*r["source_" + a]) for a in "xyz"])
        dist, az, el = random.uniform(*r["mic_distance"]), random.uniform(0.0, 2.0 * math.pi), random.uniform(-math.pi / 2, math.pi / 2)
        source = np.clip(source, WALL_MARGIN, size - WALL_MARGIN)
        mic = source + dist * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        mic = np.clip(mic, WALL_MARGIN, size - WALL_MARGIN)
        if float(np.abs(mic - source).max()) < 1e-3:
            mic[0] += 0.15 if source[0] < size[0] / 2 else -0.15
        return size, source, mic, absorption

    def draw(self):
        names = {g: False for g in STAGES}
        row = none_table(self.cap)
        if "crush" in self.p and random.random() < self.p["crush"]:
            names["crush"], row[0] = True, float(random.randint(*self.bit_range))
        if "room" in self.p and random.random() < self.p["room"]:
            size, source, mic, absorption = self.draw_room()
            ir = room_ir(size, source, mic, absorption, self.room["max_order"], self.sample_rate)
            if ir.shape[0] > self.cap:
                raise RuntimeError(f"room_ir gave {ir.shape[0]} taps for a table of {self.cap}")
            names["room"], row[1] = True, float(ir.shape[0])
            row[2:2 + ir.shape[0]] = ir
        return names, row
