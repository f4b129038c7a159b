"""Index helpers of the packed Schur partial slabs (kba_items.hpp: slab_packed_write / slab_packed_read / slab_packed_base) as a
stand-alone host program (tests/cpp/test_slab_layout.cpp), built under -fsanitize=address: writer and reader agree, every place of a
slab is hit exactly once, nothing leaves the slab or the window's region - for every system size that occurs."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_packed_slab_index_helpers():
    out = os.path.join(_HERE, "cpp", "_build", "test_slab_layout")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-ffp-contract=off", "-std=c++17", "-o", out,
                           os.path.join(_HERE, "cpp", "test_slab_layout.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout and "AddressSanitizer" not in r.stderr
    n_sys = int(r.stdout.strip().splitlines()[-1].split()[0])
    assert n_sys >= 25  # nfq 0, 6 .. 24 with 0 .. 4 plane blocks behind them (nf <= 40), and the larger pose-only systems
