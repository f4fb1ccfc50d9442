"""The key-per-voice polyphony tests' data, shared by tests/test_polyphony_reference.py, tests/test_cpp_keyfan.py,
tests/test_gpu_keyfan.py and tests/test_gpu_polyphony_player.py; holds no tests.  A case is a key table, a table capacity, stray
mask bits and a script of key events for every player over six consecutive buffers of 256 frames; the model
(tests/polyphony_reference.py) runs it once per case for the largest player count and every test slices what it needs -- player
p's script does not depend on the player count.  Voice v = player * n_keys + key."""
import functools
from dataclasses import dataclass

import numpy as np

from tests import polyphony_reference as pr

f32 = np.float32
OUT_LEN = 256
BUFFERS = 6
PLAYERS = 66                                       # what the model runs: the GPU tests take 1 and 65 of them, the C++ one all
OUTER_SPANS = 34                                   # what zang_amd.polyphony gives the outer bank: 32 impulses + the carried note + 1


@dataclass(frozen=True)
class Case:
    name: str
    n_keys: int
    max_spans: int
    seed: int
    stray: int = 0                                 # bits ORed into every pushed mask: none of them may reach a voice

    def key_freqs(self):
        """ascending from a4 = 220 in semitones (examples/common.zig's rel_freq are such steps), rounded to f32"""
        return (220.0 * 2.0 ** (np.arange(self.n_keys) / 12.0)).astype(f32)


CASES = [
    Case("keys41", 41, 34, 21),                                        # the reference's keyboard (common.key_bindings.len)
    Case("one_key", 1, 34, 22),                                        # key 0 == key n_keys - 1
    Case("keys64", 64, 34, 23),                                        # both mask words, bit 63
    Case("stray_bits", 5, 34, 24, stray=(1 << 5) | (1 << 40) | (1 << 63)),   # bits at n_keys and above it, in both words
    Case("overflow", 41, 2, 25),                                       # max_spans far too small: rows dropped and counted
]
CASE_IDS = [c.name for c in CASES]


def script(case, player):
    """-> per buffer, the player's key events [(key_index, down, frame)] in push order (frames ascending).
    buffer 0: key a down -- at frame 0 for the even players, at frame 100 for the odd ones
    buffer 1: two more keys change, at 50 and at 120: a's rows split at both
    buffer 2: a down and an up of one key, at 60 and 200
    buffer 3: two events on one frame (the first one's sub-span is empty: its mask reaches no key), then one more
    buffer 4: 33 events, seven frames apart: the outer queue holds 32, the 33rd is dropped (its key stays in the mask that the next
              buffer's events push)
    buffer 5: players 0 mod 3: silence (the carried notes play on); the others: up to four random events
    With one key a, b, c and d are all key 0: a `down` of a key that is down changes no voice but still splits the rows."""
    rng = np.random.default_rng([case.seed, player])
    n = case.n_keys
    a, b, c, d = 0, n - 1, (player * 7 + 3) % n, (player * 5 + 11) % n
    out = [[(a, True, 0 if player % 2 == 0 else 100)],
           [(b, True, 50), (c, True, 120)],
           [(d, True, 60), (d, False, 200)],
           [(a, False, 77), (b, False, 77), (c, player % 2 == 1, 255)]]
    held = set()
    evs = []
    for i in range(33):
        key = int(rng.integers(0, n))
        down = key not in held and len(held) < 6
        (held.add if down else held.discard)(key)
        evs.append((key, down, i * 7 + (player % 5)))
    out.append(evs)
    evs = []
    if player % 3:
        for frame in sorted(int(x) for x in rng.integers(0, OUT_LEN, int(rng.integers(0, 5)))):
            evs.append((int(rng.choice([a, b, int(rng.integers(0, n))])), bool(rng.random() < 0.5), frame))
    out.append(evs)
    assert len(out) == BUFFERS
    return out


@dataclass
class Run:
    """the model's record of one case: per buffer and player the pushes, the outer sub-spans, and per VOICE the inner sub-spans
    and the state words after the buffer"""
    pushed: list                                   # [buffer][player] -> [(frame, note_id, mask)] as keyEvent pushed them
    outer: list                                    # [buffer][player] -> [(s, e, mask, changed)]
    inner: list                                    # [buffer][voice] -> [(s, e, (freq, note_on), changed)]
    words: list                                    # [buffer][voice] -> zh_keyfan_state's fields, freq as bits


@functools.lru_cache(maxsize=None)
def run(case, n_players=PLAYERS):
    players = [pr.MainModule(case.key_freqs()) for _ in range(n_players)]
    scripts = [script(case, p) for p in range(n_players)]
    rec = Run([], [], [], [])
    for b in range(BUFFERS):
        pushed, outer, inner, words = [], [], [], []
        for p, pl in enumerate(players):
            pushed.append([(frame,) + pl.key_event(key, down, frame, case.stray) for key, down, frame in scripts[p][b]])
            o, i = pl.schedule(OUT_LEN)
            outer.append(o); inner += i; words += [v.words() for v in pl.polyphony.voices]
        rec.pushed.append(pushed); rec.outer.append(outer); rec.inner.append(inner); rec.words.append(words)
    return rec


def voices_of(per_voice, case, n_players):
    """the first n_players players' share of a [voice] list"""
    return per_voice[:n_players * case.n_keys]


def state_array(words, dtype):
    """[voice] word lists -> a zh_keyfan_state array (freq from its bits)"""
    st = np.zeros(len(words), dtype)
    for v, w in enumerate(words):
        st["next_id"][v], st["down"][v], st["has_note"][v], st["note_id"][v] = w[:4]
        st["freq"][v] = np.array([w[4]], np.uint32).view(f32)[0]
        st["note_on"][v] = w[5]
    return st


def state_words(st):
    """a zh_keyfan_state array -> [voice] word lists"""
    fb = np.ascontiguousarray(st["freq"]).view(np.uint32)
    return [[int(st["next_id"][v]), int(st["down"][v]), int(st["has_note"][v]), int(st["note_id"][v]), int(fb[v]), int(st["note_on"][v])]
            for v in range(len(st))]
