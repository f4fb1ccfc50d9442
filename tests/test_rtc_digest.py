"""CPU: zh_version() carries the digest of the runtime headers embedded in the library (tools/embed_headers.py), which is what
keys the on-disk cache of compiled script kernels (zang_amd/script.py): a library with other headers gets another key."""
import ctypes as C
import importlib.util
import os
import re
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zang_amd", "csrc")
INC = os.path.join(CSRC, "rtc_headers.inc")


def _tool():
    spec = importlib.util.spec_from_file_location("embed_headers", os.path.join(ROOT, "tools", "embed_headers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _written(inc):
    text = open(inc).read()
    names = re.search(r"kRtcHeaderNames\[\] = \{(.*?)\};", text).group(1)
    return re.search(r'#define ZH_RTC_DIGEST "([0-9a-f]{16})"', text).group(1), re.findall(r'"([^"]+)"', names)


def test_version_carries_the_digest_the_generator_wrote():
    from zang_amd import abi
    assert os.path.exists(abi.LIB_PATH) and os.path.exists(INC), "build libzang_hip.so first (__graft_entry__.build())"
    lib = C.CDLL(abi.LIB_PATH)
    lib.zh_version.restype = C.c_char_p
    digest, names = _written(INC)
    assert lib.zh_version().decode() == "zang_hip 0.1 (gfx950) rt:" + digest
    # ... and it is the digest of the headers as the tree holds them: the library is not older than its runtime headers
    assert "script_rt.hip.h" in names and "span_walk.hip.h" in names
    assert _tool().digest([(n, open(os.path.join(CSRC, n)).read()) for n in names]) == digest


def test_one_flipped_byte_of_a_header_changes_the_digest(tmp_path):
    tool = _tool()
    names = ["common.hip.h", "script_rt.hip.h"]
    for n in names:
        shutil.copy(os.path.join(CSRC, n), tmp_path / n)
    args = ["%s=%s" % (n, tmp_path / n) for n in names]
    tool.main(str(tmp_path / "a.inc"), args)
    raw = bytearray((tmp_path / names[1]).read_bytes())
    at = raw.index(b"zs_span_walk")
    raw[at] ^= 0x01
    (tmp_path / names[1]).write_bytes(bytes(raw))
    tool.main(str(tmp_path / "b.inc"), args)
    a, b = _written(str(tmp_path / "a.inc")), _written(str(tmp_path / "b.inc"))
    assert a[1] == b[1] == names and a[0] != b[0]
    # the name is part of it too: the same text under another name is another header set
    assert tool.digest([("x.h", "text")]) != tool.digest([("y.h", "text")])
