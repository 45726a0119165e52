"""What the layout-and-entry-point tests and the scratch-free tests share: a C program compiled against include/neo_mpc.h and
linked against libneo_mpc.so, and the compiler's resource remarks for a HIP source.  No GPU needed; a helper, not a test."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "neo_mpc_planner2_amd")
HEADER = os.path.join(ROOT, "include", "neo_mpc.h")


def run_c_probe(tmp_path, source, werror=()):
    """Compiles `source` against include/ (implicit declarations and each of `werror` are errors) and links it against
    libneo_mpc.so: what it names is declared AND exported.  Runs it -> its `name value` lines as {name: value text}."""
    src, obj, exe = tmp_path / "probe.c", tmp_path / "probe.o", tmp_path / "probe"
    src.write_text(source)
    errors = ["-Werror=" + w for w in ("implicit-function-declaration",) + tuple(werror)]
    subprocess.check_call(["gcc", "-Wall"] + errors + ["-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)])
    subprocess.check_call(["gcc", str(obj), "-L", PACKAGE, "-lneo_mpc", "-Wl,-rpath," + PACKAGE, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", str(exe)])
    return dict(line.split(None, 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())


def kernel_resources(tmp_path, hip_source, extra_flags=()):
    """The compiler's resource remarks for `hip_source`, compiled for gfx950 with the Makefile's flags and `extra_flags`,
    csrc/ on the include path -> {function: {field: int}}, the fields among them "ScratchSize", "VGPRs", "Occupancy"."""
    (tmp_path / "unit.hip").write_text(hip_source)
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                          "-Wno-pass-failed"] + list(extra_flags) + ["-Rpass-analysis=kernel-resource-usage", "-I",
                          os.path.join(PACKAGE, "csrc"), "-x", "hip", "-c", str(tmp_path / "unit.hip"), "-o", os.devnull],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    return rows
