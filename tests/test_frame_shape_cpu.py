"""The one copy of a frame row's shape (csrc/frame_shape.h): St, the row's
bytes, max_len, a frame's span on the air and the refusals, and the launch
arithmetic of the row walk (csrc/frame_rows.h), held to counts written from the
definitions in a stand-alone program under AddressSanitizer and UBSan
(tests/native/frame_shape_test.c). The program is built from the headers and
the library's host C files, whose public functions the span is compared with;
it loads no shared library.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "audio-network_amd", "csrc")
HOST_C = ["demod_fec.c", "demod_frame_check.c", "demod_tx_frame.c", "demod_frame.c"]


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frame_shape_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "frame_shape_test.c")] + [os.path.join(CSRC, f) for f in HOST_C] +
                   ["-lm", "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frame_shape_test OK: 336 combinations" in r.stdout
