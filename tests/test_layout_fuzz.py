"""CPU: the host-side layout builders under AddressSanitizer + UBSan on randomised matrices (sanitizers run on the
CPU build only; the GPU pool has none)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_builders_under_sanitizers(tmp_path):
    exe = str(tmp_path / "layout_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-pthread", os.path.join(ROOT, "tools", "layout_fuzz.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_layout_builder_threads_under_thread_sanitizer(tmp_path):
    """The builder classifies rows, runs both counting sorts and tiles the fragments on several host threads; the same
    randomised matrices under ThreadSanitizer (fewer trials: it is slow), layouts compared with the one-thread build."""
    exe = str(tmp_path / "layout_fuzz_tsan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-fno-omit-frame-pointer", "-pthread",
                    os.path.join(ROOT, "tools", "layout_fuzz.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "10", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_layout_digests_match_golden(tmp_path):
    """Bit for bit: `layout_fuzz digest` builds the TILED layout of a fixed corpus of matrices and knob settings and prints,
    per case, build_tiled's return code and an FNV-1a digest of every array, counter and unit table it produced.  The
    lines must equal tests/golden/layout_digests.txt, recorded from the builder as it was before it was cut into stages.
    A deliberate layout change regenerates the file (from the repository root):

        mkdir -p build && g++ -std=c++17 -O2 -pthread tools/layout_fuzz.cpp -o build/layout_fuzz && build/layout_fuzz digest > tests/golden/layout_digests.txt
    """
    exe = str(tmp_path / "layout_fuzz_digest")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", os.path.join(ROOT, "tools", "layout_fuzz.cpp"), "-o", exe], check=True)
    knobs = ("EMSAR_HIP_", "EMSAR_HOST_THREADS")
    env = {k: v for k, v in os.environ.items() if not k.startswith(knobs)}
    r = subprocess.run([exe, "digest"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "layout_digests.txt")) as f:
        want = f.read().splitlines()
    got = r.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w, "the layout of case %s moved: got '%s', recorded '%s'" % (w.split()[0], g, w)
    assert len(got) == len(want), "%d cases printed, %d recorded" % (len(got), len(want))
