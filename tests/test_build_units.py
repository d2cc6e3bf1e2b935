"""CPU-only checks of the build's unit list (lightning_amd/_build.py): what a translation unit depends on is derived from its #include lines, so
a header edit rebuilds the units that see it and no other; and no .hip file of csrc/ is left out of the library."""
import os

from lightning_amd import _build


def _names(src):
    return {os.path.basename(p) for p in _build.unit_deps(src)}


def test_unit_dependencies_follow_the_includes():
    store = _names("lamd_store.hip")
    assert "store_digest.h" in store
    assert "fe.h" in store  # through engine_internal.h -> verify_core.h -> group.h
    core = _names("lamd_engine.hip")
    assert "store_digest.h" not in core and "bolt11.h" not in core
    assert {"engine_internal.h", "verify_core.h", "fe.h", "fe_asm.inc"} <= core
    for src, _ in _build.ENGINE_TUS:
        for dep in _build.unit_deps(src):
            assert os.path.isfile(dep) and dep.startswith(_build.ROOT + os.sep)


def test_every_hip_file_is_a_unit():
    units = {src for src, _ in _build.ENGINE_TUS}
    on_disk = {f for f in os.listdir(_build.CSRC) if f.endswith(".hip")}
    assert on_disk - {"lamd_testgen.hip"} == {u for u in units if u.endswith(".hip")}
    # one flag list for every unit with device code: the mul24 workaround reaches each of them
    for src, flags in _build.ENGINE_TUS:
        if src.endswith(".hip"):
            assert flags == _build.HIPFLAGS + _build.EXTRA and "-amdgpu-codegenprepare-mul24=false" in flags
