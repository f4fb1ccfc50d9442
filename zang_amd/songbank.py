"""A bank of songs rendered at once: example_song's MainModule + write_wav's buffer loop (examples/example_song.zig:287-396,
examples/write_wav.zig:58-93) for N songs, with no host work per song.

Per instrument of the song format (Pedal, RegularOrgan, WeirdOrgan) the bank holds ONE voice bank of N instruments (instrument i
= song i's events, zang_amd.bank), ONE module object of N * polyphony voices and ONE image [frames][N * polyphony].  A batch of
buffers is: per instrument a schedule launch and a paint_spans launch; then the grouped mixdown chain (zang.mixdownGroups /
mixdownGroupsPcm) -- every song's sub-voices added in the reference's painting order (:340-346) and converted by zang.mixDown in
the last link -- and one copy of the [N][frames * 2] s16 block to the host.  Every payload has the bits SongRenderer gives that
song alone.

With `echoes=(main_delay, feedback_volume, cutoff)` every song's mix goes through the output bus effect of example_delay.zig:69-79,
StereoEchoes(main_delay), before mixDown: the bank owns ONE StereoEchoes of N voices (voice = song).  A batch then mixes every
instrument into the f32 rows, turns them into a [frames][N] image, paints the echoes once over the batch (the delays and the
constant-parameter filter do not depend on where a span is cut) into a left and a right image, and converts each with
mixdownGroupsPcm (groups of one voice, channels 0 and 1) into one [N][frames * 4] block of interleaved stereo s16.
"""
import numpy as np

from . import zang
from .bank import VoiceBank
from .song import (AUDIO_BUFFER_SIZE, AUDIO_SAMPLE_RATE, EXAMPLE_SONG_INSTRUMENTS, MyNoteParams, NativeSongScheduler, compile_song,
                   resolve_frequencies)


class SongBank:
    """`songs`: N per-instrument event lists, each what resolve_frequencies(compile_song(text), ctx) returns."""

    def __init__(self, ctx, songs, instruments=EXAMPLE_SONG_INSTRUMENTS, vol=0.25, echoes=None):
        from . import modules as mod
        if not songs:
            raise ValueError("SongBank: at least one song")
        if any(len(s) != len(instruments) for s in songs):
            raise ValueError("SongBank: every song holds one event list per instrument")
        self.ctx, self.instruments, self.vol = ctx, instruments, vol
        self.n_songs = N = len(songs)
        self.banks, self.mods = [], []
        for k, inst in enumerate(instruments):
            evs = [e for s in songs for e in s[k]]
            offsets = np.concatenate([[0], np.cumsum([len(s[k]) for s in songs])]).astype(np.uint64)
            rec = np.zeros(len(evs), NativeSongScheduler._dtype)
            # makeParams (example_song.zig:35-39 etc.): freq * freq_mul in f32, once per event
            rec["freq"] = np.array([e.freq for e in evs], np.float32) * np.float32(inst.freq_mul)
            rec["note_on"] = [e.note_on for e in evs]
            self.banks.append(VoiceBank(ctx, inst.polyphony, rec, offsets, [e.t for e in evs], [e.note_id for e in evs],
                                        MyNoteParams.note_on.offset, rows=34))
            cls = mod.PMOscInstrument if inst.kind == "pmosc" else mod.NiceInstrument
            self.mods.append(cls(N * inst.polyphony, inst.init_arg, ctx))
        self.echoes, self._echo_params = None, None
        if echoes is not None:
            main_delay, feedback_volume, cutoff = echoes
            self.echoes = mod.StereoEchoes(N, int(main_delay), ctx)
            self._echo_params = (float(feedback_volume), float(cutoff))
        self._channels = 2 if self.echoes is not None else 1
        self._rows = 34
        self._frames = 0
        self._pcm = {}                                              # batch frames -> [N][frames * 2] uint8 (one contiguous block to copy)
        self._rewind = None                                         # (states before the stream's short last buffer, its frames)
        self.trace_kernels = False                                  # True: render_batch notes the kernels of its launches in last_kernels
        self.last_kernels = []

    @classmethod
    def from_texts(cls, ctx, texts, instruments=EXAMPLE_SONG_INSTRUMENTS, vol=0.25, echoes=None):
        return cls(ctx, [resolve_frequencies(compile_song(t, instruments), ctx) for t in texts], instruments, vol, echoes)

    def _reserve(self, counts):
        import torch
        total = int(sum(counts))
        rows = 33 * len(counts) + 1                                 # <= 32 impulses + carry-over per buffer per sub-voice
        if rows > self._rows:
            for b in self.banks:
                b.reserve(rows)
            self._rows = rows
        if total > self._frames:
            self._images = [self.ctx.image(total, self.n_songs * i.polyphony) for i in self.instruments]
            self._mix = torch.zeros((self.n_songs, total), dtype=torch.float32, device=self.ctx.device)
            if self.echoes is not None:                             # the bus: [frames][songs] input, left and right
                self._bus = [self.ctx.image(total, self.n_songs) for _ in range(3)]
            self._frames = total
        if total not in self._pcm:
            self._pcm[total] = torch.zeros((self.n_songs, total * 2 * self._channels), dtype=torch.uint8, device=self.ctx.device)
        return total

    def render_batch(self, frame_counts):
        """Several consecutive write_wav iterations of every song, from the state the bank is in (a short last buffer of an
        earlier render() stays as it was rendered): -> uint8 array [N][sum(frame_counts) * 2] of s16 mono PCM ([N][... * 4],
        interleaved stereo, with echoes)."""
        self._rewind = None
        return self._render_batch(frame_counts)

    def _render_batch(self, frame_counts):
        counts = [int(n) for n in frame_counts]
        total = self._reserve(counts)
        if total == 0:
            return np.zeros((self.n_songs, 0), np.uint8)
        span, sr = zang.Span(0, total), float(AUDIO_SAMPLE_RATE)
        self.last_kernels = []
        note = (lambda: self.last_kernels.extend(self.ctx.last_form())) if self.trace_kernels else (lambda: None)
        for bank, m, img in zip(self.banks, self.mods, self._images):
            bank.schedule(counts, sr, self._rows)
            note()
            m.paint_spans(span, [img[:total]], None, sr, bank.span_table(self._rows, MyNoteParams.freq.offset // 4), zero_first=True)
            note()
        pcm, last = self._pcm[total], len(self.instruments) - 1
        if self.echoes is not None:
            return self._finish_with_echoes(span, total, pcm, note)
        for k, (inst, img) in enumerate(zip(self.instruments, self._images)):     # outputs[0] zeroed, then `+=` in painting order
            if k < last:
                zang.mixdownGroups(span, self._mix, img[:total], inst.polyphony, zero_first=(k == 0), ctx=self.ctx)
            else:
                zang.mixdownGroupsPcm(span, pcm, img[:total], inst.polyphony, zang.AudioFormat.signed16_lsb, 1, 0, self.vol,
                                      acc=self._mix if k else None, ctx=self.ctx)
            note()
        return pcm.cpu().numpy()

    def _finish_with_echoes(self, span, total, pcm, note):
        """the batch's output half with the bus effect: f32 rows -> [frames][songs] image -> StereoEchoes -> two PCM channels"""
        for k, (inst, img) in enumerate(zip(self.instruments, self._images)):     # outputs[0] zeroed, then `+=` in painting order
            zang.mixdownGroups(span, self._mix, img[:total], inst.polyphony, zero_first=(k == 0), ctx=self.ctx)
            note()
        bus_in, left, right = (b[:total] for b in self._bus)
        bus_in.copy_(self._mix[:, :total].t())
        fb, cutoff = self._echo_params
        self.echoes.paint(span, [left, right], None, False, self.echoes.Params(bus_in, fb, cutoff), zero_first=True)
        note()
        for ch, img in enumerate((left, right)):                                  # write_wav.zig:71-78, one call per channel
            zang.mixdownGroupsPcm(span, pcm, img, 1, zang.AudioFormat.signed16_lsb, 2, ch, self.vol, ctx=self.ctx)
            note()
        return pcm.cpu().numpy()

    def render(self, seconds, batch=8):
        """write_wav's loop (write_wav.zig:58-93; the last buffer may be short), `batch` buffers per set of launches: -> N `bytes`
        of s16 mono PCM (interleaved stereo with echoes).
        Calls continue ONE stream whose buffers stay on its 1,024-frame grid.  A short last buffer is rendered as write_wav
        renders it, but the state it started from is kept: the next call goes back to it, renders that buffer again at the
        length it now has and leaves out the frames already handed over.  So every buffer but the stream's very last one is
        scheduled and painted whole, whatever the calls' lengths (NoteTracker's clock and the PMOsc's phase wrap both depend on
        where the buffers are cut: a 46 x 1,024 + 896 cut twice is not a 93 x 1,024 + 768 cut)."""
        skip = 0
        if self._rewind is not None:
            (banks, mods, echo), skip = self._rewind
            for b, st in zip(self.banks, banks):
                b.set_state(st)
            for m, st in zip(self.mods, mods):
                m.set_state(st)
            if self.echoes is not None:
                self.echoes.set_state(*echo)
            self._rewind = None
        total = skip + int(seconds * AUDIO_SAMPLE_RATE)
        counts, start = [], 0
        while start < total:                                        # write_wav.zig:58-59
            n = min(AUDIO_BUFFER_SIZE, total - start)
            counts.append(n)
            start += n
        short = bool(counts) and counts[-1] < AUDIO_BUFFER_SIZE
        whole_buffers = counts[:-1] if short else counts
        blocks = [self._render_batch(whole_buffers[i:i + batch]) for i in range(0, len(whole_buffers), batch)]
        if short:
            self._rewind = (([b.get_state() for b in self.banks], [m.state() for m in self.mods],
                             self.echoes.state() if self.echoes is not None else None), counts[-1])
            blocks.append(self._render_batch(counts[-1:]))
        if not blocks:
            return [b""] * self.n_songs
        out = np.concatenate(blocks, axis=1)[:, skip * 2 * self._channels:]
        return [out[i].tobytes() for i in range(self.n_songs)]

    def overflows(self):
        """sub-spans the banks dropped so far because a voice's list was full (must stay 0; synchronises)"""
        return sum(b.overflows() for b in self.banks)

    def close(self):
        for b in self.banks:
            b.close()
        self.banks = []
        if self.echoes is not None:
            self.echoes.close()
            self.echoes = None
