"""GPU box: the spans form (zs_paint_spans_<name>) of random zangscript modules (tests/script_fuzz.py) over random per-voice
sub-span tables with random per-sub-span params, against oracle/zs_interp.py voice by voice, bit for bit, then one ordinary
paint from the state the spans left.  usage: fuzz_script_spans.py N [first_seed]   (70 voices, 96-frame buffers)"""
import os, sys
os.environ["ZH_ENV_LIVE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zang_amd
from tests import script_fuzz
from tests.test_gpu_script_spans import _parity
ctx = zang_amd.default_context()
n = int(sys.argv[1]); first = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
bad = 0
for seed in range(first, first + n):
    text, name = script_fuzz.generate(seed)
    try:
        _parity(ctx, text, "fuzz", name, 70, seed, buffers=2, Fb=96)
    except AssertionError as e:
        bad += 1; print("FAIL seed", seed, str(e)[:2000]); print(text)
    except Exception as e:
        bad += 1; print("ERROR seed", seed, type(e).__name__, str(e)[:2000]); print(text)
print("seeds", n, "from", first, "failures", bad)
sys.exit(1 if bad else 0)
