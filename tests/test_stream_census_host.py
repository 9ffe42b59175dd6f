"""sr_stream_census needs no GPU: a process that has made no coefficient call has made no stream."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_accepts_null_pointers():
    from spectrobot_amd._lib import lib
    assert lib.sr_stream_census(None, None) == 0
    live = C.c_int(-1)
    assert lib.sr_stream_census(C.byref(live), None) == 0 and live.value >= 0
    total = C.c_int(-1)
    assert lib.sr_stream_census(None, C.byref(total)) == 0 and total.value >= live.value


def test_fresh_process_has_no_streams():
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from spectrobot_amd._lib import lib; a, b = C.c_int(-1), C.c_int(-1); "
            "assert lib.sr_stream_census(C.byref(a), C.byref(b)) == 0; print(a.value, b.value)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["0", "0"]
