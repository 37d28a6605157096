"""Writes tests/golden/codec_golden.npz: what CPython's audioop (standard library up to Python 3.12) makes of the inputs the codec tests
use.  Run once, by hand, under a Python that still has audioop; the tests read the npz alone.

  ulaw_encode, alaw_encode   uint8 [65536]: lin2ulaw / lin2alaw of every int16 value, entry s + 32768
  ulaw_decode, alaw_decode   int16 [256]: ulaw2lin / alaw2lin of every code
  adpcm_<kind>_<L>_x         int16 [L]: a row of kind "uniform" (seeded), "sine" (windowed) or "square" (seeded, +-full scale)
  adpcm_<kind>_<L>_codes     uint8 [L]: lin2adpcm's codes, one per sample, the high nibble of a byte first.  An odd L: one zero sample is
                             appended before encoding (audioop drops an unpaired nibble; the encoder is causal) and L codes are kept
  adpcm_<kind>_<L>_decoded   int16 [L]: adpcm2lin of those bytes, the first L samples
  adpcm_<kind>_<L>_state     int32 [2]: lin2adpcm's final (val, idx) on exactly the L samples
"""
import os

import numpy as np

ADPCM_LENGTHS = (0, 1, 2, 7, 64, 65, 1001, 4096)
ADPCM_KINDS = ("uniform", "sine", "square")


def adpcm_row(kind, L):
    rng = np.random.default_rng(7000 + 10 * L + ADPCM_KINDS.index(kind))
    if kind == "uniform":
        return rng.integers(-32768, 32768, L).astype(np.int16)
    n = np.arange(L)
    if kind == "sine":
        w = 0.5 - 0.5 * np.cos(2 * np.pi * (n + 0.5) / max(L, 1))
        return np.rint(30000.0 * w * np.sin(2 * np.pi * 440.0 * n / 8000.0)).astype(np.int16)
    period = rng.integers(3, 40)
    return np.where((n // period + rng.integers(0, 2)) % 2 == 0, 32767, -32768).astype(np.int16)


def main():
    import audioop
    out = {}
    every = np.arange(-32768, 32768, dtype=np.int16)
    codes = bytes(range(256))
    out["ulaw_encode"] = np.frombuffer(audioop.lin2ulaw(every.tobytes(), 2), np.uint8).copy()
    out["alaw_encode"] = np.frombuffer(audioop.lin2alaw(every.tobytes(), 2), np.uint8).copy()
    out["ulaw_decode"] = np.frombuffer(audioop.ulaw2lin(codes, 2), np.int16).copy()
    out["alaw_decode"] = np.frombuffer(audioop.alaw2lin(codes, 2), np.int16).copy()
    for kind in ADPCM_KINDS:
        for L in ADPCM_LENGTHS:
            x = adpcm_row(kind, L)
            even = np.concatenate([x, np.zeros(L % 2, np.int16)])
            packed, _ = audioop.lin2adpcm(even.tobytes(), 2, None)
            _, state = audioop.lin2adpcm(x.tobytes(), 2, None)
            b = np.frombuffer(packed, np.uint8)
            nibbles = np.stack([b >> 4, b & 15], axis=1).reshape(-1)
            decoded, _ = audioop.adpcm2lin(packed, 2, None)
            key = "adpcm_%s_%d_" % (kind, L)
            out[key + "x"] = x
            out[key + "codes"] = nibbles[:L].astype(np.uint8)
            out[key + "decoded"] = np.frombuffer(decoded, np.int16)[:L].copy()
            out[key + "state"] = np.array(state, np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "codec_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
