"""What the layout-and-entry-point tests and the scratch-free tests share: a C program compiled against include/neo_mpc.h and
linked against libneo_mpc.so, and the compiler's resource remarks for a HIP source.  No GPU needed; a helper, not a test."""
import ctypes as C
import os
import re
import subprocess

from neo_mpc_planner2_amd import _lib, abi

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


def probe_header(tmp_path, records=(), constants=(), entry_points=()):
    """The probe generated from names alone, compiled, linked and run: for every C struct of `records` its sizeof and the
    offsetof of every field its Python mirror names, the value of every NEO_MPC_<constant>, and every entry point taken by
    address -> {"sizeof.<struct>": n, "<struct>.<field>": offset, "<constant>": value}."""
    body = ""
    for name in records:
        body += '  printf("sizeof.%s %%zu\\n", sizeof(%s));\n' % (name, name)
        body += "".join('  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (name, f, name, f)
                        for f, _ in abi.RECORDS[name].struct._fields_)
    body += "".join('  printf("%s %%u\\n", (unsigned)NEO_MPC_%s);\n' % (c, c) for c in constants)
    body += "  void* volatile f[] = {(void*)neo_mpc_abi_version%s};\n" % "".join(", (void*)" + n for n in entry_points)
    body += "  for (size_t i = 0; i < sizeof f / sizeof f[0]; ++i) if (f[i] == 0) return 1;\n  return 0;\n"
    got = run_c_probe(tmp_path, '#include <stdio.h>\n#include <stddef.h>\n#include "neo_mpc.h"\nint main(void) {\n' + body + "}\n")
    return {k: int(v) for k, v in got.items()}


def check_layout(got, c_name, size, struct=None, dtype=None):
    """`got` (probe_header's) against abi.RECORDS[c_name]: the header's sizeof equals both mirrors' and the literal `size`; for
    every field the header's offsetof equals the ctypes offset and the dtype's; the dtype names the struct's fields in order.
    `struct` / `dtype`: the public names of abi that must be those mirrors."""
    record = abi.RECORDS[c_name]
    assert struct in (None, record.struct) and (dtype is None or dtype is record.dtype), c_name
    assert got["sizeof." + c_name] == C.sizeof(record.struct) == record.dtype.itemsize == record.size == size, c_name
    fields = [f for f, _ in record.struct._fields_]
    assert list(record.dtype.names) == fields, c_name
    for f in fields:
        assert got["%s.%s" % (c_name, f)] == getattr(record.struct, f).offset == record.dtype.fields[f][1], (c_name, f)


def check_entry_points(names):
    """Every one of `names` is declared by the header as `int name(`, listed in _lib.EXPORTS and exported by the library; the
    header and the library are at ABI version 2, behaviour version 6."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert "#define NEO_MPC_ABI_VERSION 2" in text and "#define NEO_MPC_BEHAVIOUR_VERSION 6" in text
    assert _lib.load().neo_mpc_abi_version() == 2 and _lib.load().neo_mpc_behaviour_version() == 6


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
