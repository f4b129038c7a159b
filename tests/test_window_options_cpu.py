"""The host rule of per-window solve options (limo_amd/csrc/kba_window_options.hpp: which fields of limo_ba_options may differ between
the windows of one batch, the error text per field, all-equal gives no table, a record's bytes against make_consts of its entry) as a
stand-alone host program (tests/cpp/test_window_options.cpp), built under -fsanitize=address together with kba_pack.cpp."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_window_options_rule_and_records():
    out = os.path.join(_HERE, "cpp", "_build", "test_window_options")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-ffp-contract=off", "-std=c++17", "-pthread", "-o", out,
                           os.path.join(_HERE, "cpp", "test_window_options.cpp"), os.path.join(_HERE, "..", "limo_amd", "csrc", "kba_pack.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed checks" in r.stdout and "AddressSanitizer" not in r.stderr
    # 17 fixed fields x 4 checks, 4 free fields x (3 + 6 refusals x 2), 5 records x 7: the count guards against a run that checked nothing
    assert int(r.stdout.strip().splitlines()[-1].split()[0]) >= 17 * 4 + 4 * 3 + 4 * 12 + 5 * 7
