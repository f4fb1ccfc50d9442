"""The visualiser's spectrum widgets for every voice of an image at once (zh_spectrum_plot / zh_spectrum_column, csrc/spectrum.hip):
what the reference's example harness does with each MainModule's output_visualize buffer, 1,024 frames at a time
(examples/visual.zig: DrawSpectrum :211-330, DrawSpectrumFull :363-458, over examples/common/fft.zig).  Both read fft_real only,
as the reference does.  Spectrum is the 512-row magnitude plot; Spectrogram keeps DrawSpectrumFull's scrolling state."""
import ctypes as C

import torch

from . import abi
from .runtime import as_buf

FRAMES = 1024           # what both plots take (visual.zig:261, :421)
BINS = 512


def fft(ctx, re, im, n=None, frame_start=0):
    """fft(n, re, im) of examples/common/fft.zig for every voice, in place on rows [frame_start, frame_start + n) of both images"""
    n = re.shape[0] - frame_start if n is None else n
    abi.check(ctx.lib.zh_fft(ctx.handle, int(n), int(frame_start), as_buf(re), as_buf(im)), "zh_fft")


class Spectrum:
    """DrawSpectrum.plot for `voices` columns: plot(image) -> the [512][voices] tensor of sqrt(|fft_real| / 1024), overwritten by
    every plot (the reference assigns)."""

    def __init__(self, ctx, voices):
        self.ctx, self.voices = ctx, int(voices)
        self.out = ctx.image(BINS, self.voices, fill=0.0)         # fft_out starts zeroed (visual.zig:245)

    def plot(self, image, frame_start=0):
        abi.check(self.ctx.lib.zh_spectrum_plot(self.ctx.handle, int(frame_start), as_buf(image), as_buf(self.out)), "zh_spectrum_plot")
        return self.out


class Spectrogram:
    """DrawSpectrumFull for `voices` columns: a [height][width][voices] buffer of pixel words (0xAABBGGRR as int32 bits), one
    column per plot at `drawindex`, which advances and wraps at `width` (visual.zig:443-449); a change of `logarithmic` zeroes the
    buffer and resets drawindex first (:415-419).  scrolled() is the picture in time order, as scrollBlit draws it (:127-139)."""

    def __init__(self, ctx, voices, width, height):
        if height < 2 or width < 1:
            raise ValueError("a spectrogram needs height >= 2 (the reference divides by height - 1) and width >= 1")
        self.ctx, self.voices, self.width, self.height = ctx, int(voices), int(width), int(height)
        self.logarithmic = False                                  # :397-398
        self.drawindex = 0
        self.buffer = torch.zeros((self.height, self.width, self.voices), dtype=torch.int32, device=ctx.device)

    def _column(self, image, frame_start):
        ptr = self.buffer.data_ptr() + 4 * self.drawindex * self.voices
        abi.check(self.ctx.lib.zh_spectrum_column(self.ctx.handle, int(frame_start), as_buf(image), C.c_void_p(ptr), self.width * self.voices,
                                                  self.height, 1 if self.logarithmic else 0), "zh_spectrum_column")

    def plot(self, image, frame_start=0, logarithmic=False):
        logarithmic = bool(logarithmic)
        if self.logarithmic != logarithmic:
            self.logarithmic = logarithmic
            self.buffer.zero_()
            self.drawindex = 0
        self._column(image, frame_start)
        self.drawindex += 1
        if self.drawindex == self.width:
            self.drawindex = 0
        return self.buffer

    def scrolled(self):
        """[height][width][voices] with the oldest column first: buffer columns drawindex.. followed by ..drawindex"""
        return torch.roll(self.buffer, -self.drawindex, dims=1)
