"""Builds liblightning_amd.so (+ the host mirror and the test-traffic library) in-tree with hipcc for gfx950 (cross-compiles without a GPU).

One object per translation unit under lightning_amd/build/, then one link: a change to the gossip_store headers recompiles lamd_store.hip, not
the ecmult kernels of lamd_engine.hip; stale units compile side by side.  What a unit depends on is read from its #include "..." lines,
followed through the tree.  Staleness is decided by CONTENT: every artefact has a stamp file holding the sha256 of its sources, its flags and
its inputs' stamps; file times play no part (a snapshot copied to the GPU box keeps the stamps next to the libraries, so nothing is rebuilt
there).

python -m lightning_amd._build variant NAME FLAGS...: the engine with extra compile flags as tools/variants/liblightning_amd_NAME.so
(tools/build_variant.sh)."""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
OBJDIR = os.path.join(PKG, "build")
LIB = os.path.join(PKG, "liblightning_amd.so")
INC = os.path.join(ROOT, "include")
_H = lambda *names: [os.path.join(CSRC, f) for f in names]
_I = lambda *names: [os.path.join(INC, f) for f in names]

# -amdgpu-codegenprepare-mul24=false: ROCm 7.2's AMDGPUCodeGenPrepare mul24 rewrite miscompiles the fused
# 64-bit column arithmetic of fe.h (a^2*a came out wrong on gfx950; reproduced instruction-for-instruction by
# an ISA emulator, so it is a code-generation bug, not a hardware hazard -- DESIGN.md "toolchain notes").
# lamd_selftest() re-checks every primitive on the device against the host evaluation of the same code.
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wno-unknown-pragmas", "-mllvm", "-amdgpu-codegenprepare-mul24=false"]
EXTRA = os.environ.get("LAMD_BUILD_FLAGS", "").split()

_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def includes(path, seen=None):
    """every file of this tree that `path` includes, directly or through another header (sorted; `path` itself is not in the list)"""
    seen = {} if seen is None else seen
    with open(path, encoding="utf-8", errors="replace") as f:
        text = f.read()
    for name in _INCLUDE.findall(text):
        dep = os.path.normpath(os.path.join(os.path.dirname(path), name))
        if dep not in seen and dep.startswith(ROOT + os.sep) and os.path.exists(dep):
            seen[dep] = True
            includes(dep, seen)
    return sorted(seen)


# translation units of liblightning_amd.so and their flags: every unit with device code takes the ONE HIPFLAGS list (the mul24 workaround reaches
# each of them).  lamd_engine.hip: the core; lamd_store.hip: the gossip_store calls; lamd_frontends.hip: transactions, TLV streams and text in front
# of the core; lamd_debug.hip: the debuggers.  (lamd_testgen.hip is a library of its own, below.)
MULTI_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-pthread", "-Wall"]
ENGINE_TUS = [(src, HIPFLAGS + EXTRA) for src in ("lamd_engine.hip", "lamd_store.hip", "lamd_frontends.hip", "lamd_debug.hip")] + [("lamd_multi.cpp", MULTI_FLAGS)]
MAX_COMPILES = 16


def unit_deps(src):
    return includes(os.path.join(CSRC, src))


# test / bench infrastructure: the synthetic-workload signer kernels (include/lightning_amd_testgen.h)
TESTGEN = os.path.join(PKG, "liblightning_amd_testgen.so")
TESTGEN_SOURCES = _H("lamd_testgen.hip") + includes(os.path.join(CSRC, "lamd_testgen.hip"))

SHIM = os.path.join(PKG, "liblightning_amd_cln.so")
SHIM_CPP = _H("cln_shim.cpp", "gossip_ingest.cpp")
SHIM_SOURCES = SHIM_CPP + _I("cln_shim.h", "lightning_amd_gossipd.h", "lightning_amd.h") + _H("verify_core.h")


def _digest(files, extra=()):
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    for e in extra:
        h.update(str(e).encode() + b"\0")
    return h.hexdigest()


def _fresh(artefact, digest):
    try:
        return os.path.exists(artefact) and open(artefact + ".stamp").read().strip() == digest
    except OSError:
        return False


def _stamp(artefact, digest):
    with open(artefact + ".stamp", "w") as f:
        f.write(digest + "\n")


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _engine_digests():
    return [(src, _digest([os.path.join(CSRC, src)] + unit_deps(src), flags), flags) for src, flags in ENGINE_TUS]


def _jobs(n):
    """concurrent compiles: one per stale unit, MAX_COMPILES at the most, MAX_JOBS where the environment sets it"""
    try:
        limit = int(os.environ.get("MAX_JOBS", ""))
    except ValueError:
        limit = MAX_COMPILES
    return max(1, min(n, MAX_COMPILES, limit))


def _compile_units(units, verbose=False):
    """units: (command, object, digest); each object is stamped as it lands.  A unit that fails does not stop the others: its error is raised when
    they have finished (their objects and stamps stay, so the next build compiles the failed unit alone); verbose command lines may interleave"""
    def one(u):
        cmd, obj, digest = u
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(obj + ".tmp", obj)
        if digest:
            _stamp(obj, digest)
    if units:
        with ThreadPoolExecutor(max_workers=_jobs(len(units))) as pool:
            list(pool.map(one, units))


def _link(objs, out, verbose=False):
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", out] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)


def is_stale():
    tus = _engine_digests()
    return not _fresh(LIB, _digest([], [d for _, d, _ in tus]))


def build_shim(force=False):
    """host-side C++ mirror of the reference prototypes + the gossip ingest (links against liblightning_amd.so)"""
    digest = _digest(SHIM_SOURCES, ["shim-v2"])
    if not force and _fresh(SHIM, digest) and os.path.exists(LIB):
        return SHIM
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-o", SHIM + ".tmp"] + SHIM_CPP +
                          ["-L" + PKG, "-llightning_amd", "-Wl,-rpath,$ORIGIN"])
    os.replace(SHIM + ".tmp", SHIM)
    _stamp(SHIM, digest)
    return SHIM


def build_testgen(force=False):
    digest = _digest(TESTGEN_SOURCES, HIPFLAGS)
    if not force and _fresh(TESTGEN, digest) and os.path.exists(LIB):
        return TESTGEN
    subprocess.check_call([_hipcc()] + [f for f in HIPFLAGS if f != "-pthread"] + ["-shared", "-o", TESTGEN + ".tmp", os.path.join(CSRC, "lamd_testgen.hip"),
                           "-L" + PKG, "-llightning_amd", "-Wl,-rpath,$ORIGIN"])
    os.replace(TESTGEN + ".tmp", TESTGEN)
    _stamp(TESTGEN, digest)
    return TESTGEN


# the shared-service front (include/lightning_amd_served.h): host code only -- the server binds the engine through dlopen, the client speaks
# to the server; liblightning_amd_cln_client.so is the mirror linked against the CLIENT instead of the engine
SERVED = os.path.join(PKG, "lamd_served")
CLIENT = os.path.join(PKG, "liblightning_amd_client.so")
SHIM_CLIENT = os.path.join(PKG, "liblightning_amd_cln_client.so")
SERVED_SOURCES = _H("lamd_served.cpp", "served_common.h", "numa_cpus.h") + _I("lightning_amd_served.h", "lightning_amd.h")
CLIENT_SOURCES = _H("lamd_client.cpp", "served_common.h") + _I("lightning_amd_served.h", "lightning_amd.h")


def build_served(force=False):
    """lamd_served + liblightning_amd_client.so + liblightning_amd_cln_client.so (g++, seconds; no device code)"""
    cxx = os.environ.get("CXX", "g++")
    flags = ["-O2", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    d = _digest(SERVED_SOURCES, ["served-v1"])
    if force or not _fresh(SERVED, d):
        subprocess.check_call([cxx] + flags + ["-o", SERVED + ".tmp", os.path.join(CSRC, "lamd_served.cpp"), "-ldl"])
        os.replace(SERVED + ".tmp", SERVED)
        _stamp(SERVED, d)
    d = _digest(CLIENT_SOURCES, ["client-v2"])
    if force or not _fresh(CLIENT, d):
        # -Bsymbolic-functions: the library's own calls (lamd_check_signed_hash -> lamd_verify_ecdsa_batch) bind inside it even in a process that has the
        # engine library's symbols of the same names in its global scope
        subprocess.check_call([cxx] + flags + ["-shared", "-Wl,-Bsymbolic-functions", "-o", CLIENT + ".tmp", os.path.join(CSRC, "lamd_client.cpp")])
        os.replace(CLIENT + ".tmp", CLIENT)
        _stamp(CLIENT, d)
    d = _digest(SHIM_SOURCES + CLIENT_SOURCES, ["shim-client-v1"])
    if force or not _fresh(SHIM_CLIENT, d):
        subprocess.check_call([cxx] + flags + ["-shared", "-o", SHIM_CLIENT + ".tmp"] + SHIM_CPP + ["-L" + PKG, "-llightning_amd_client", "-Wl,-rpath,$ORIGIN"])
        os.replace(SHIM_CLIENT + ".tmp", SHIM_CLIENT)
        _stamp(SHIM_CLIENT, d)
    return SERVED, CLIENT, SHIM_CLIENT


def build(force=False, verbose=False):
    tus = _engine_digests()
    link_digest = _digest([], [d for _, d, _ in tus])
    if not force and _fresh(LIB, link_digest):
        build_shim()
        build_testgen()
        build_served()
        return LIB
    os.makedirs(OBJDIR, exist_ok=True)
    objs, stale = [], []
    for src, digest, flags in tus:
        obj = os.path.join(OBJDIR, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if force or not _fresh(obj, digest):
            stale.append(([_hipcc()] + flags + ["-c", "-o", obj + ".tmp", os.path.join(CSRC, src)], obj, digest))
    _compile_units(stale, verbose)
    _link(objs, LIB + ".tmp", verbose)
    os.replace(LIB + ".tmp", LIB)
    _stamp(LIB, link_digest)
    build_shim(force=True)
    build_testgen()
    build_served()
    return LIB


def build_variant(name, extra):
    """the engine's units with `extra` behind their own flags, linked into tools/variants/liblightning_amd_NAME.so: the shipped library, its objects
    and its stamps are not touched"""
    out = os.path.join(ROOT, "tools", "variants")
    os.makedirs(out, exist_ok=True)
    objs, units = [], []
    for src, flags in ENGINE_TUS:
        obj = os.path.join(out, "%s_%s.o" % (os.path.splitext(src)[0], name))
        objs.append(obj)
        units.append(([_hipcc()] + flags + (extra if src.endswith(".hip") else []) + ["-c", "-o", obj + ".tmp", os.path.join(CSRC, src)], obj, None))
    _compile_units(units, verbose=True)
    lib = os.path.join(out, "liblightning_amd_%s.so" % name)
    _link(objs, lib, verbose=True)
    for obj in objs:
        os.remove(obj)
    return lib


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "variant":
        print(build_variant(sys.argv[2], sys.argv[3:]))
    else:
        sys.exit("usage: python -m lightning_amd._build variant NAME [FLAGS...]")
