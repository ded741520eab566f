"""The gfx950 code object of a built object file, the kernel descriptors of an AMDGPU
ELF, and what the Makefile says of the build (its flags, its objects): the one extractor,
the one parser and the one place that asks make, shared by the *_builds.py tests,
test_build_recipe.py, test_scene_table.py and tools/co_diff.py.  Plain helpers, no
fixtures."""
import os
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd", "build")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def make_words(var):
    """The words of the Makefile's variable `var`, as make expands it."""
    r = subprocess.run(["make", "-s", "--no-print-directory", "--eval", f"print-var: ; @echo $({var})", "print-var"],
                       cwd=ROOT, capture_output=True, text=True, check=True)
    return r.stdout.split()


def hipflags():
    """The Makefile's HIPFLAGS, the flags every object of librm is compiled with."""
    flags = make_words("HIPFLAGS")
    assert "-ffp-contract=off" in flags, flags
    return flags


def kernel_objects(but=()):
    """The objects of librm that hold kernels (the Makefile's RM_KERNEL_OBJS, which
    test_build_recipe.py holds against the build), as file names, except those in `but`."""
    return [o + ".o" for o in make_words("RM_KERNEL_OBJS") if o + ".o" not in but]


def gfx950_code_object(obj_path, work_dir):
    """The bytes of the one gfx950 code object bundled in the host object obj_path
    (llvm-objdump --offloading writes it next to a copy of the object, in work_dir)."""
    os.makedirs(work_dir, exist_ok=True)
    shutil.copy(obj_path, os.path.join(work_dir, "x.o"))
    subprocess.run([OBJDUMP, "--offloading", "x.o"], cwd=work_dir, capture_output=True, check=True)
    cos = [p for p in os.listdir(work_dir) if "gfx950" in p]
    assert len(cos) == 1, os.listdir(work_dir)
    with open(os.path.join(work_dir, cos[0]), "rb") as f:
        return f.read()


def kernel_descriptors(co):
    """{kernel: dict(lds, scratch, vgprs, sgprs, offset, size)} of every kernel in an AMDGPU
    ELF, from its 64-byte descriptor `<kernel>.kd`: group_segment_fixed_size (LDS bytes; u32
    at offset 0), private_segment_fixed_size (scratch bytes per lane; u32 at offset 4) and the
    allocations compute_pgm_rsrc1 (offset 48) encodes on gfx950: bits 5:0 (granule + 1) * 8 of
    the unified vector file per lane, bits 9:6 (granule / 2 + 1) * 16 scalar registers.  offset
    and size place the kernel's code in the file (its function symbol)."""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]
    syms = {}
    for _, type_, _, _, off, size, link, _, _, _ in secs:
        if type_ != 2:  # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for k in range(size // 24):
            st_name, _, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", co, off + 24 * k)
            if 0 < st_shndx < shnum:
                sym = co[stroff + st_name:co.index(b"\0", stroff + st_name)].decode()
                sec = secs[st_shndx]
                syms[sym] = (sec[4] + (st_value - sec[3]), st_size)
    out = {}
    for sym, (kd, _) in syms.items():
        if not sym.endswith(".kd"):
            continue
        lds, scratch = struct.unpack_from("<II", co, kd)
        rsrc1, = struct.unpack_from("<I", co, kd + 48)
        offset, size = syms.get(sym[:-3], (0, 0))
        out[sym[:-3]] = dict(lds=lds, scratch=scratch, vgprs=((rsrc1 & 63) + 1) * 8,
                             sgprs=(((rsrc1 >> 6) & 15) // 2 + 1) * 16, offset=offset, size=size)
    return out


def built_descriptors(obj, tmp_path):
    """kernel_descriptors of the gfx950 code object in the in-tree build's object `obj`."""
    import pytest
    src = os.path.join(BUILD, obj)
    if not os.path.exists(src):
        pytest.skip("librm not built")
    return kernel_descriptors(gfx950_code_object(src, str(tmp_path / obj)))


def field(kd, name):
    """{kernel: its descriptor's field `name`}."""
    return {k: v[name] for k, v in kd.items()}


def private_sizes(obj, tmp_path):
    """{kernel: scratch bytes per lane} of the in-tree build's object `obj`."""
    return field(built_descriptors(obj, tmp_path), "scratch")
