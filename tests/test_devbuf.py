"""rr::DevBuf, the owner of every device allocation of the engine (csrc/rr_devbuf.hpp), without a GPU: the header reaches the device through
two functions it only declares, so a small stand-alone program (devbuf_main.cpp) defines them over malloc / free and drives the type under
AddressSanitizer + UndefinedBehaviorSanitizer -- destructor, moves (onto a non-empty buffer, onto itself), release BEFORE allocate, reserve,
a refused allocation, count <= 0, arrays and a growing vector, nothing alive at the end.  The program links the sanitizer itself."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_devbuf_under_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler on the path'
    exe = str(tmp_path / 'devbuf')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-I', os.path.join(ROOT, 'river_route_amd', 'csrc'),
                    '-o', exe, os.path.join(HERE, 'devbuf_main.cpp')], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == '', f'exit {r.returncode}\n{r.stdout}\n{r.stderr}'
    assert r.stdout.split()[2:] == ['live', '0', 'failures', '0']
