"""The arpeggiator tests' data, shared by tests/test_arp_reference.py, tests/test_cpp_arp.py, tests/test_gpu_arp.py and
tests/test_gpu_arp_player.py; holds no tests.  A case is a sample rate (hence a note_duration), a key table, a table capacity and
a seeded script of key events for every player over six consecutive buffers; the model (tests/arp_reference.py) runs it once per
case for the largest player count and every test slices what it needs -- player p's script does not depend on the player count."""
import functools
from dataclasses import dataclass

import numpy as np

from tests import arp_reference as ar

f32 = np.float32
OUT_LEN = 256
BUFFERS = 6
PLAYERS = [1, 63, 64, 65, 200]
OUTER_SPANS = 34                                   # what zang_amd.arp gives the outer bank: 32 impulses + the carried note + 1
REJECTED_RATES = [0.0, 33.0, float("nan"), float("inf"), -48000.0, 1e12]   # 33: 0.03f * 33 = 0.99 truncates to 0


def search_f32_rate(lo=2900, hi=4000):
    """the first integer sample rate in [lo, hi) whose note_duration differs when the product of the same f32 constant is made in
    f64: f32(0.03) is 0.0299999993..., so rate * it falls just short of an integer that the f32 product rounds up to"""
    for sr in range(lo, hi):
        if ar.note_duration(float(sr)) != ar.note_duration_f64(float(sr)):
            return sr
    return None


# search_f32_rate() == 2900 (tests/test_arp_reference.py runs the search): 0.03f * 2900 is 87 in f32 and 86.999998 in f64
F32_RATE = 2900.0


@dataclass(frozen=True)
class Case:
    name: str
    sample_rate: float
    n_keys: int
    max_spans: int
    seed: int
    max_events: int = 5                            # key events per player and buffer: 0 .. max_events

    @property
    def note_duration(self):
        return ar.note_duration(self.sample_rate)

    def key_freqs(self):
        """ascending, most inside the PulseOsc's range [0, sample_rate / 8], the top tenth above it"""
        return (np.linspace(0.01, 0.135, self.n_keys) * self.sample_rate).astype(f32)


CASES = [
    Case("nd1_one_key", 40.0, 1, 256, 11, max_events=2),           # 256 ticks a call: the queue's cap; n_keys 1: index 0 == n_keys - 1
    Case("nd7", 240.0, 39, 256, 12),                               # 37 ticks a call: the cap again
    Case("nd100", 3334.0, 64, 64, 13),
    Case("nd300", 10001.0, 64, 64, 14),                            # note_duration > out_len: buffers without a tick
    Case("f32_product", F32_RATE, 39, 64, 15),                     # 87, where an f64 product gives 86
    Case("overflow", 240.0, 39, 5, 16),                            # max_spans far too small: rows dropped and counted
]
CASE_IDS = [c.name for c in CASES]
EXPECTED_ND = {"nd1_one_key": 1, "nd7": 7, "nd100": 100, "nd300": 300, "f32_product": 87, "overflow": 7}


def script(case, player):
    """-> per buffer, the player's key events [(key_index, down, frame)] in push order (frames ascending).  Held keys never exceed
    five.  Buffer 0: players 0 mod 4 begin with key 0 down at frame 0; players 1 mod 4 have no event at all (the arpeggiator must
    not run before the first one) and begin in buffer 1 with the LAST key down at frame out_len - 1.  Buffer 3 releases every held
    key at one frame (equal frames), buffer 4 is silent for the even players (note-offs tick on), odd ones play on."""
    rng = np.random.default_rng([case.seed, player])
    held, out = [], []
    n = case.n_keys
    for b in range(BUFFERS):
        evs = []
        if b == 0 and player % 4 == 1:
            out.append(evs)
            continue
        if b == 3:
            frame = int(rng.integers(0, OUT_LEN))
            evs = [(k, False, frame) for k in held]
            held = []
            out.append(evs)
            continue
        if b == 4 and player % 2 == 0:
            out.append(evs)
            continue
        k = int(rng.integers(0, case.max_events + 1))
        pool = [0, OUT_LEN - 1] + [int(x) for x in rng.integers(0, OUT_LEN, 3)]
        frames = sorted(int(rng.choice(pool)) for _ in range(k))       # equal frames are likely: five picks of at most five values
        for i, frame in enumerate(frames):
            down = len(held) < 5 and (not held or rng.random() < 0.6)
            if down:
                key = int(rng.choice([0, n - 1, int(rng.integers(0, n))]))
                if key not in held:
                    held.append(key)
            else:
                key = held.pop(int(rng.integers(0, len(held))))
            evs.append((key, down, frame))
        if b == 0 and player % 4 == 0:
            evs = [(0, True, 0)] + [e for e in evs if e[0] != 0]
        if b == 1 and player % 4 == 1:
            evs = [(n - 1, True, OUT_LEN - 1)]
        if (b, player % 4) in ((0, 0), (1, 1)):                        # the events were replaced: nothing was held before them
            held = []
            for key, down, _ in evs:
                if down and key not in held:
                    held.append(key)
                elif not down and key in held:
                    held.remove(key)
        out.append(evs)
    return out


@dataclass
class Run:
    """the model's record of one case: per buffer and player the outer and the inner sub-spans and the state words after it"""
    outer: list                                    # [buffer][player] -> [(s, e, held list, changed)]
    inner: list                                    # [buffer][player] -> [(s, e, (freq, note_on), changed)]
    words: list                                    # [buffer][player] -> zh_arp_state's fields
    stats: list                                    # [player] -> the arpeggiator's counters at the end
    pushed: list                                   # [buffer][player] -> [(frame, note_id, mask)] as keyEvent pushed them


@functools.lru_cache(maxsize=None)
def run(case, n_players=max(PLAYERS)):
    players = [ar.Player(case.key_freqs()) for _ in range(n_players)]
    scripts = [script(case, p) for p in range(n_players)]
    rec = Run([], [], [], [], [])
    for b in range(BUFFERS):
        outer, inner, words, pushed = [], [], [], []
        for p, pl in enumerate(players):
            pushed.append([(frame,) + pl.key_event(key, down, frame) for key, down, frame in scripts[p][b]])
            o, i = pl.schedule(OUT_LEN, case.sample_rate)
            outer.append(o); inner.append(i); words.append(pl.arp.words())
        rec.outer.append(outer); rec.inner.append(inner); rec.words.append(words); rec.pushed.append(pushed)
    rec.stats = [pl.arp.stats for pl in players]
    return rec


def mask_of(held):
    return sum(1 << i for i, h in enumerate(held) if h)


def state_array(words, dtype):
    """[player] word lists -> a zh_arp_state array (freq from its bits)"""
    st = np.zeros(len(words), dtype)
    for p, w in enumerate(words):
        st["next_frame"][p], st["next_id"][p], st["last_note"][p], st["has_note"][p], st["note_id"][p] = w[:5]
        st["freq"][p] = np.array([w[5]], np.uint32).view(f32)[0]
        st["note_on"][p] = w[6]
    return st


def state_words(st):
    """a zh_arp_state array -> [player] word lists"""
    return [[int(st["next_frame"][p]), int(st["next_id"][p]), int(st["last_note"][p]), int(st["has_note"][p]), int(st["note_id"][p]),
             int(st["freq"][p:p + 1].view(np.uint32)[0]), int(st["note_on"][p])] for p in range(len(st))]
