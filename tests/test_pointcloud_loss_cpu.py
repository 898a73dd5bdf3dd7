"""CPU: the per-point body of the point-cloud loss (diffsdfsim_amd/csrc/pointcloud_point.h: geom.h on Dual<6> and the hand-written
chain from the body-frame point to the pose) against a long double restatement of phi^2 and long double central differences
for its ten derivatives, 2 000 random points per primitive (tests/emu/check_pointcloud_loss.cpp, a program of its own, built
with the address and undefined-behaviour sanitizers where g++ has their runtimes)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pointcloud_point_terms_equal_long_double_value_and_central_differences():
    out = os.path.join(HERE, "emu", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "check_pointcloud_loss")
    cmd = ["g++", "-O1", "-std=c++17", "-w", "-I", os.path.join(HERE, "emu"), "-o", exe, os.path.join(HERE, "emu", "check_pointcloud_loss.cpp")]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)      # (no sanitizer runtimes on this machine)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    w = r.stdout.split()
    cases, inside, worst_value, worst_deriv = int(w[0]), int(w[1]), float(w[3]), float(w[5])
    # six primitives x 2 000 points; both sides of the query cube are well represented
    assert cases == 12000 and 6000 < inside < cases, r.stdout
    assert worst_value < 1e-12 and worst_deriv < 1e-9, r.stdout
