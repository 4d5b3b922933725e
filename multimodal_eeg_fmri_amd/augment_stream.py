"""The augmenters' random stream, host side (csrc/aug_stream.h is the device side; DESIGN.md 5i defines both): the stream
words the kernels take as arguments, and the numpy replica the CPU paths of `EEGTransforms`, `EEGTimeTransforms` and
`VolumeTransforms` draw with.  Counter based: a pure function of (seed, step, rank, purpose, index), no state anywhere."""
import numpy as np

# purpose number = position in this table; each augmenter owns one run, so the three are independent at equal seed and step
PURPOSES = {
    "eeg": ("noise_decision", "drop_decision", "channel_keys", "gauss_a", "gauss_b"),
    "volume": ("flip_decision", "shift_decision", "shift_z", "shift_y", "shift_x", "scale_decision", "scale_u",
               "noise_decision", "gauss_a", "gauss_b", "erase_decision", "erase_z", "erase_y", "erase_x"),
    "eeg_time": ("shift_decision", "shift_amount", "scale_decision", "scale_u", "invert_decision", "mask_decision",
                 "mask_start"),
}
_M64 = (1 << 64) - 1


def stream_word(seed: int, step: int, rank: int, purpose: int) -> int:
    """stream(seed, step, rank, purpose): 64-bit arithmetic mod 2^64, folded to 32 bits"""
    z = (int(seed) * 0x9E3779B97F4A7C15 + int(step) * 0xBF58476D1CE4E5B9 + int(rank) * 0x94D049BB133111EB
         + (purpose + 1) * 0xD6E8FEB86659FD93) & _M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & _M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & _M64
    z ^= z >> 31
    return (z ^ (z >> 32)) & 0xFFFFFFFF


def streams(owner: str, seed: int, step: int, rank: int = 0) -> tuple:
    """the 32-bit stream words of one step of augmenter ``owner``, in the order of its purposes"""
    owners = list(PURPOSES)
    first = sum(len(PURPOSES[o]) for o in owners[:owners.index(owner)])
    return tuple(stream_word(seed, step, rank, first + k) for k in range(len(PURPOSES[owner])))


def aug_hash(stream: int, idx: np.ndarray) -> np.ndarray:
    """h(stream, idx) on a uint64 array of 32-bit indices -> uint64 array of 32-bit values"""
    m = np.uint64(0xFFFFFFFF)
    x = (idx.astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(stream)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x + np.uint64(((stream << 16) | (stream >> 16)) & 0xFFFFFFFF)) & m
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def aug_thresh(p: float) -> int:
    """decision threshold of a probability, formed through double from its fp32 value (as the kernels' host code does)"""
    p = float(np.float32(p))
    return 0 if p <= 0.0 else 1 << 32 if p >= 1.0 else int(p * 4294967296.0)


def sample_draws(owner: str, seed: int, step: int, rank: int, B: int) -> dict:
    """{purpose name: h(stream, b) for b in range(B)}: the per-sample draws of one step of augmenter ``owner``"""
    b = np.arange(B, dtype=np.uint64)
    return {name: aug_hash(s, b) for name, s in zip(PURPOSES[owner], streams(owner, seed, step, rank))}


def decide(h: np.ndarray, p: float) -> np.ndarray:
    """decision on  iff  h < thresh(p)"""
    return h < np.uint64(aug_thresh(p))


def uniform(h: np.ndarray, n: int) -> np.ndarray:
    """uniform integer in [0, n): (h * n) >> 32"""
    return ((h * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def scale_factor(scale_range: float, h: np.ndarray) -> np.ndarray:
    """fp32( 1 + (double)scale_range * (h * 2^-31 - 1) ) of the fp32 value ``scale_range``"""
    return (1.0 + float(np.float32(scale_range)) * (h.astype(np.float64) * 2.0 ** -31 - 1.0)).astype(np.float32)


def gauss_field(stream_a: int, stream_b: int, first_pair: int, n_pairs: int) -> np.ndarray:
    """the unit Gaussians of Box-Muller pairs first_pair .. first_pair + n_pairs - 1, fp64 (2 * n_pairs,): pair idx gives
    sqrt(-2 ln u1) * (cos, sin)(2 pi u2) with u1 = (h(stream_a, idx) + 1) * 2^-32 in (0, 1], u2 = h(stream_b, idx) * 2^-32"""
    idx = np.uint64(first_pair) + np.arange(n_pairs, dtype=np.uint64)
    u1 = (aug_hash(stream_a, idx).astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = aug_hash(stream_b, idx).astype(np.float64) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=-1).reshape(-1)


class StepCounter:
    """what the three augmenters share as dataset transforms: the per-sample ``__call__`` takes its step index from a call
    counter, which - with the seed - is the augmenter's state"""
    calls = 0

    def next_step(self) -> int:
        step, self.calls = self.calls, self.calls + 1
        return step

    def state_dict(self) -> dict:
        return {"seed": self.seed, "calls": self.calls}

    def load_state_dict(self, sd: dict) -> None:
        self.seed, self.calls = int(sd["seed"]), int(sd["calls"])
