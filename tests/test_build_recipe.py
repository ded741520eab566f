"""The one recipe every librm is built by (Makefile): the in-tree build, a variant
(tools/build_variant.sh, which runs make) and the host sanitizer build (`make asan`) are
one static pattern rule over RM_OBJS with BUILD, LIBRM, XFLAGS, KOPT, RM_PIXEL_SLP and
SAN set.  All checks but the last two read `make -n -B` dry runs: which commands a
setting gives, not what they compile to.  The last two hold the recipe against the
in-tree build: each kernel is in one object, and a plain variant built through the
script has the in-tree build's kernels byte for byte.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from code_objects import BUILD, OBJDUMP, ROOT, gfx950_code_object, kernel_descriptors, kernel_objects, make_words

PKG = "opengl-raymarching-in-compute-shader_amd"
SCRIPT = os.path.join(ROOT, "tools", "build_variant.sh")
PROBES = ["MARCH", "BMARCH", "NORMAL", "SHADOW", "LIGHT", "GAMMA", "CAST", "STORE"]
SANHOST = ("-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined "
           "-Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer").split()


def commands(text):
    """The command lines of a dry run's output, each as its tokens."""
    return [line.split() for line in text.replace("\\\n", " ").splitlines() if line.strip()]


def dry(*args):
    r = subprocess.run(["make", "-n", "-B", "--no-print-directory", *args], cwd=ROOT, capture_output=True,
                       text=True, check=True)
    return commands(r.stdout)


def after(tokens, flag):
    return tokens[tokens.index(flag) + 1]


def compiles(cmds):
    """{object name: its compile's tokens}; no object is compiled twice."""
    out = {}
    for t in cmds:
        if "-c" in t and "-o" in t:
            name = os.path.basename(after(t, "-o"))[:-2]
            assert name not in out, name
            out[name] = t
    return out


def links(cmds):
    return [t for t in cmds if "-shared" in t and after(t, "-o").endswith("librm.so")]


def defines(tokens):
    return sorted(t for t in tokens if t.startswith("-D"))


@pytest.fixture(scope="module")
def plain():
    return dry("librm")


def test_librm_is_one_compile_per_object_and_one_link(plain):
    objs = make_words("RM_OBJS")
    assert len(objs) == len(set(objs)) and set(kernel_objects()) <= {o + ".o" for o in objs}
    assert sorted(compiles(plain)) == sorted(objs)
    link, = links(plain)
    assert [t for t in link if t.endswith(".o")] == [f"{PKG}/build/{o}.o" for o in objs]
    assert after(link, "-o") == f"{PKG}/librm.so"


def test_build_and_librm_move_every_output():
    cmds = dry("librm", "BUILD=/x/objs", "LIBRM=/y/librm.so")
    comp = compiles(cmds)
    assert comp and all(after(t, "-o") == f"/x/objs/{o}.o" for o, t in comp.items())
    assert "-I/x/objs" in comp["rm_jit"]
    embed, = [t for t in cmds if any(w.endswith("embed_sources.py") for w in t)]
    assert embed[2] == "/x/objs/rm_jit_src.inc", embed
    link, = links(cmds)
    assert after(link, "-o") == "/y/librm.so"
    assert all(t.startswith("/x/objs/") for t in link if t.endswith(".o"))
    assert not [t for c in cmds for t in c if f"{PKG}/build" in t], "something still goes to the default directory"


def test_xflags_reach_every_compile_and_change_nothing_else(plain):
    base, comp = compiles(plain), compiles(dry("librm", "XFLAGS=-DRM_DBL_MARCH=1"))
    assert sorted(comp) == sorted(base)
    for o, t in comp.items():
        assert t.count("-DRM_DBL_MARCH=1") == 1, (o, t)
        assert [w for w in t if w != "-DRM_DBL_MARCH=1"] == base[o], o


def test_xflags_replace_the_sample_kernels_defaults(plain):
    assert {"-DRM_LEAN_FIXED_WORK=1", "-DRM_FAST_STEPS=1"} <= set(compiles(plain)["rm_kernels_aa"])
    aa = compiles(dry("librm", "XFLAGS=-DRM_FAST_STEPS=0"))["rm_kernels_aa"]
    assert [t for t in aa if "RM_FAST_STEPS" in t] == ["-DRM_FAST_STEPS=0"], aa
    assert aa.count("-DRM_LEAN_FIXED_WORK=1") == 1, aa


def test_kopt_and_pixel_slp_change_the_built_in_kernels_flags_only(plain):
    base, comp = compiles(plain), compiles(dry("librm", "KOPT=-O3", "RM_PIXEL_SLP=1"))
    assert [o for o, t in base.items() if "-O2" in t]
    for o, t in base.items():
        want = ["-O3" if w == "-O2" else w for w in t]
        if o == "rm_kernels":
            want[want.index("-fno-slp-vectorize")] = "-fslp-vectorize"
        assert comp[o] == want, o


def test_stats_build_has_one_object_of_rm_kernels():
    cmds = dry("librm", "XFLAGS=-DRM_STATS=1")
    comp = compiles(cmds)
    assert "rm_kernels_aa" not in comp
    assert defines(comp["rm_kernels"]) == ["-DRM_STATS=1"], comp["rm_kernels"]
    link, = links(cmds)
    assert not [t for t in link if "rm_kernels_aa" in t]
    assert [t for t in link if t.endswith("/rm_kernels.o")]


def test_asan_is_the_same_rule_in_its_sanitizer_mode(plain):
    base, cmds = compiles(plain), dry("asan")
    comp = compiles(cmds)
    assert sorted(comp) == sorted(base)
    for o, t in comp.items():
        assert after(t, "-c") == after(base[o], "-c"), o
        assert defines(t) == defines(base[o]), o
        assert after(t, "-o") == f"{PKG}/build/asan/{o}.o"
        if t[0].endswith("hipcc"):
            at = [i for i in range(len(t)) if t[i:i + len(SANHOST)] == SANHOST]
            assert len(at) == 1, t
            levels = [i for i, w in enumerate(t) if re.fullmatch(r"-O\w", w)]
            assert t[levels[-1]] == "-O1" and "-g" in t, t
        else:  # rm_host.cpp has no device side: clang++ with the sanitizers as such
            assert o == "rm_host" and t[0].endswith("clang++") and "-fsanitize=address,undefined" in t, t
    assert "-I" + f"{PKG}/build/asan" in comp["rm_jit"]
    assert not [c for c in cmds if re.search(re.escape(PKG) + r"/build(?!/asan)", " ".join(c))]
    link, = links(cmds)  # the two outputs are where test_sanitizers.py looks for them
    assert after(link, "-o") == f"{PKG}/build/asan/librm.so" and "-shared-libsan" in link
    assert [c for c in cmds if "-o" in c and after(c, "-o") == "oracle/_build/librm_oracle_asan.so"]


def run_script(script, tmp_path, *args):
    """tools/build_variant.sh with its make running dry (make reads MAKEFLAGS) and every
    output under tmp_path."""
    env = dict(os.environ, MAKEFLAGS="n", BUILD=str(tmp_path / "objs"), VARIANTS=str(tmp_path / "variants"),
               TMPDIR=str(tmp_path))
    for k in ("KOPT", "RM_PIXEL_SLP"):
        env.pop(k, None)
    return subprocess.run(["bash", script, *args], capture_output=True, text=True, env=env)


def test_script_checks_the_probes_before_it_builds(tmp_path):
    r = run_script(SCRIPT, tmp_path, "x", "-DRM_DBL_MARCHH=1")
    assert r.returncode != 0 and "unknown cost probe" in r.stderr, r.stderr
    assert "hipcc" not in r.stdout + r.stderr, "a make ran"
    flags = [f"-DRM_DBL_{p}=1" for p in PROBES]
    r = run_script(SCRIPT, tmp_path, "x", *flags)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(tmp_path / "variants" / "librm_x.so")]
    comp = compiles(commands(r.stderr))
    assert sorted(comp) == sorted(make_words("RM_OBJS"))
    for o, t in comp.items():
        assert [w for w in t if w.startswith("-DRM_DBL_")] == flags, (o, t)
        assert after(t, "-o") == str(tmp_path / "objs" / (o + ".o"))


@pytest.mark.skipif(shutil.which("git") is None, reason="git not installed")
def test_script_refuses_flags_a_revisions_recipe_would_ignore(tmp_path):
    """A revision from before XFLAGS builds by its own Makefile, which would drop the -D
    flags: a copy of the script in a repository of its own whose Makefile has none."""
    repo = tmp_path / "repo"
    os.makedirs(repo / "tools")
    shutil.copy(SCRIPT, repo / "tools" / "build_variant.sh")
    os.makedirs(repo / PKG / "csrc")
    (repo / PKG / "csrc" / "rm_api.hip").write_text("")
    (repo / "Makefile").write_text("LIBRM := librm.so\nlibrm: $(LIBRM)\n$(LIBRM):\n\ttrue hipcc -o $@\n")
    git = ["git", "-C", str(repo), "-c", "user.name=t", "-c", "user.email=t@example.org"]
    for cmd in (["init", "-q"], ["add", "Makefile", PKG], ["commit", "-q", "-m", "old"]):
        subprocess.run(git + cmd, check=True, capture_output=True)
    script = str(repo / "tools" / "build_variant.sh")
    r = run_script(script, tmp_path, "x", "--rev", "HEAD", "-DRM_DBL_MARCH=1")
    assert r.returncode != 0 and "XFLAGS" in r.stderr, r.stderr
    assert "hipcc" not in r.stdout + r.stderr, "a make ran"
    r = run_script(script, tmp_path, "x", "--rev", "HEAD")
    assert r.returncode == 0 and "hipcc" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["objs", "repo", "variants"], "the staged tree was left behind"


def code_object(path, work):
    """The gfx950 code object bundled in an object file, or None for a host-only object."""
    try:
        return gfx950_code_object(path, work)
    except (AssertionError, subprocess.CalledProcessError):
        return None


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """{object name: its gfx950 code object or None} of the in-tree build."""
    if not os.path.exists(os.path.join(BUILD, "rm_kernels.o")):
        pytest.skip("librm not built")
    work = tmp_path_factory.mktemp("co")
    return {o: code_object(os.path.join(BUILD, o + ".o"), str(work / o)) for o in make_words("RM_OBJS")}


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
def test_every_kernel_is_in_exactly_one_object(built):
    """And the objects that hold kernels are the Makefile's RM_KERNEL_OBJS, the list the
    *_builds.py tests take their "every other object" from."""
    where = {}
    for o, co in built.items():
        for k in (kernel_descriptors(co) if co else ()):
            where.setdefault(k, []).append(o)
    print(len(where), "kernels in", len({o for v in where.values() for o in v}), "objects")
    assert where and not {k: v for k, v in where.items() if len(v) != 1}
    assert sorted({v[0] + ".o" for v in where.values()}) == sorted(kernel_objects())


@pytest.mark.skipif(not os.path.exists(OBJDUMP) or not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc / llvm-objdump not installed")
def test_a_plain_variant_is_the_in_tree_build(built, tmp_path):
    """One real build through the script, objects and library under tmp_path: every
    object's code object has the in-tree build's kernels, each with the same descriptor
    fields and the same code byte for byte, and nothing is left anywhere else.  (The files
    as wholes cannot be equal: hipcc names one symbol of each, __hip_cuid_<hash>, by a
    hash of its command line, which holds the output path, and the symbol hash tables
    follow the name.)"""
    variants = os.path.join(ROOT, "tools", "variants")
    before = sorted(os.listdir(variants)) if os.path.isdir(variants) else None
    tmp = tmp_path / "tmp"
    os.makedirs(tmp)
    env = dict(os.environ, BUILD=str(tmp_path / "objs"), VARIANTS=str(tmp_path / "variants"), TMPDIR=str(tmp))
    for k in ("KOPT", "RM_PIXEL_SLP", "MAKEFLAGS"):
        env.pop(k, None)
    r = subprocess.run(["bash", SCRIPT, "plain"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split() == [str(tmp_path / "variants" / "librm_plain.so")] and os.path.exists(r.stdout.strip())
    for o, co in built.items():
        mine = code_object(str(tmp_path / "objs" / (o + ".o")), str(tmp_path / "co" / o))
        assert (mine is None) == (co is None), o
        kd, mkd = (kernel_descriptors(c) if c else {} for c in (co, mine))
        assert sorted(mkd) == sorted(kd), o
        for k, d in kd.items():
            m = mkd[k]
            assert {f: v for f, v in m.items() if f != "offset"} == {f: v for f, v in d.items() if f != "offset"}, (o, k)
            assert mine[m["offset"]:m["offset"] + m["size"]] == co[d["offset"]:d["offset"] + d["size"]], (o, k)
    assert sum(co is not None for co in built.values()) >= len(kernel_objects())
    assert os.listdir(tmp) == []
    assert (sorted(os.listdir(variants)) if os.path.isdir(variants) else None) == before
