"""The one copy of a frame row's shape (csrc/frame_shape.h): St, the row's
bytes, max_len and the refusals, held to counts written from the definitions
in a stand-alone program under AddressSanitizer and UBSan
(tests/native/frame_shape_test.c). The program includes the header alone and
links nothing from the library.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "frame_shape_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "frame_shape_test.c"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frame_shape_test OK: 336 combinations" in r.stdout
