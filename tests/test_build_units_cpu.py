"""The library is one object per source of ccfindr_amd/csrc: the Makefile, __graft_entry__.build() and the directory name the
same sources, every header is a dependency, and the linked library holds the device buffer pool ONCE (a pool definition that
slipped into a header would give every unit its own 4 GB pool)."""
import glob
import os
import re
import subprocess
import tempfile

import __graft_entry__ as g

ROOT = g.ROOT
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def on_disk(*patterns):
    return {p for pat in patterns for p in glob.glob(os.path.join(g.CSRC, pat))}


def test_the_makefile_build_and_the_directory_name_the_same_sources():
    out = subprocess.run(["make", "-n", "-B", os.path.relpath(g.LIB, ROOT)], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    link = [ln for ln in out.splitlines() if " -shared " in ln]
    assert len(link) == 1, out
    objects = re.findall(r"build/obj/(\w+)\.o", link[0])
    compiled = {os.path.join(ROOT, s) for s in re.findall(r" (ccfindr_amd/csrc/\w+\.(?:cpp|hip))$", out, flags=re.M)}
    disk = on_disk("*.cpp", "*.hip")
    assert compiled == disk == set(g.HIP_SOURCES)
    assert g.HIP_SOURCES == sorted(g.HIP_SOURCES)
    stems = sorted(os.path.splitext(os.path.basename(s))[0] for s in disk)
    assert len(set(stems)) == len(stems), "two sources would share one object"
    assert sorted(objects) == stems


def test_every_header_is_a_dependency_of_the_build():
    headers = on_disk("*.h")
    assert headers and headers <= set(g.HIP_DEPS)
    assert os.path.join(ROOT, "include", "vbnmf.h") in g.HIP_DEPS and set(g.HIP_SOURCES) <= set(g.HIP_DEPS)


def test_every_kernel_is_emitted_by_one_unit():
    """A kernel that two units emit is compiled twice and loaded twice: a non-template __global__ in a header that two units
    include, or a template that two units launch.  The names come from the metadata note of each object's gfx950 code object."""
    g.build(quiet=True)
    llvm = os.path.dirname(READELF)
    home = {}
    for obj in sorted(glob.glob(os.path.join(g.OBJ, "*.o"))):
        if ".hip_fatbin" not in subprocess.run([READELF, "-S", obj], capture_output=True, text=True, check=True).stdout:
            continue
        with tempfile.TemporaryDirectory() as d:
            fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
            subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(d, "copy.o")], check=True)
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
            if os.path.getsize(co) == 0:      # a unit without kernels
                continue
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
        for name in re.findall(r"^    \.name:\s+(\S+)$", notes, flags=re.M):      # (a kernel's own key: its arguments' sit deeper)
            home.setdefault(name, []).append(os.path.basename(obj))
    assert len(home) > 100 and len({v[0] for v in home.values()}) >= 10, sorted({v[0] for v in home.values()})
    twice = {k: v for k, v in home.items() if len(v) > 1}
    assert not twice, twice


def test_the_library_holds_one_buffer_pool():
    g.build(quiet=True)
    out = subprocess.run([READELF, "--symbols", "--demangle", "-W", g.LIB], capture_output=True, text=True, check=True).stdout
    # the static symbol table: one row per defined function, local or global (the dynamic table repeats the exported ones)
    table = [ln for ln in out.split("Symbol table '.symtab'")[1].splitlines() if " FUNC " in ln and " UND " not in ln]
    assert len(table) > 100
    for fn in ("device_pool", "pool_alloc", "dev_free"):
        rows = [ln for ln in table if re.search(r"\bvbnmf::(\(anonymous namespace\)::)?%s\(" % fn, ln)]
        assert len(rows) == 1, (fn, rows)
