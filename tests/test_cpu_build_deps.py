"""The build's staleness rule (spp-rl_amd/build.py): a unit is recompiled when its object or depfile is missing,
the depfile does not parse, or a file the depfile lists is missing or newer than the object.  Fake sources, objects
and depfiles in a temporary directory: no compiler, no GPU."""
import glob
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "spp-rl_amd"))
import build as B  # noqa: E402

T_SRC, T_OBJ, T_NEW = 1_000_000_000, 1_000_000_100, 1_000_000_200  # sources < objects < an edit


@pytest.fixture
def tree(tmp_path, monkeypatch):
    """csrc/ with two units and their headers, build/ with their objects and depfiles; everything up to date"""
    csrc, obj = tmp_path / "csrc", tmp_path / "build"
    csrc.mkdir()
    obj.mkdir()
    deps = {"ks_sac_bf16.hip": ["kset.h", "sac.hip", "sac_bf.h", "common.h"],
            "api_onp.hip": ["host.h", "onp.hip", "common.h"]}
    for unit, hs in deps.items():
        for f in [unit] + hs:
            (csrc / f).write_text("")
            os.utime(csrc / f, (T_SRC, T_SRC))
        o = obj / unit.replace(".hip", ".o")
        o.write_text("")
        # the unit by its absolute path, the headers relative to csrc/ (the compiler's working directory)
        (obj / (o.name + ".d")).write_text("%s: %s \\\n  %s\n" % (o, csrc / unit, " \\\n  ".join(hs)))
        os.utime(o, (T_OBJ, T_OBJ))
    monkeypatch.setattr(B, "CSRC", str(csrc))
    monkeypatch.setattr(B, "OBJ", str(obj))
    return csrc, obj


def stale(csrc, unit):
    return B._stale(str(csrc / unit))


def test_up_to_date_tree_is_not_stale(tree):
    csrc, _ = tree
    assert not stale(csrc, "ks_sac_bf16.hip") and not stale(csrc, "api_onp.hip")


def test_header_edit_rebuilds_exactly_the_units_that_list_it(tree):
    csrc, _ = tree
    os.utime(csrc / "sac_bf.h", (T_NEW, T_NEW))
    assert stale(csrc, "ks_sac_bf16.hip")
    assert not stale(csrc, "api_onp.hip")


def test_unit_edit_rebuilds_it(tree):
    csrc, _ = tree
    os.utime(csrc / "api_onp.hip", (T_NEW, T_NEW))
    assert stale(csrc, "api_onp.hip")
    assert not stale(csrc, "ks_sac_bf16.hip")


def test_missing_depfile_or_object_is_stale(tree):
    csrc, obj = tree
    os.remove(obj / "api_onp.o.d")
    assert stale(csrc, "api_onp.hip")
    os.remove(obj / "ks_sac_bf16.o")
    assert stale(csrc, "ks_sac_bf16.hip")


def test_unparsable_or_empty_depfile_is_stale(tree):
    csrc, obj = tree
    (obj / "api_onp.o.d").write_text("not a make rule\n")
    assert stale(csrc, "api_onp.hip")
    (obj / "ks_sac_bf16.o.d").write_text("")
    assert stale(csrc, "ks_sac_bf16.hip")


def test_depfile_naming_a_deleted_file_is_stale(tree):
    csrc, _ = tree
    os.remove(csrc / "onp.hip")
    assert stale(csrc, "api_onp.hip")
    assert not stale(csrc, "ks_sac_bf16.hip")


def test_parser_handles_continuations_and_escaped_spaces():
    text = "build/ks_dw.o: /src/ks_dw.hip \\\n  dw.hip /opt/my\\ rocm/include/hip/hip\\ runtime.h \\\n\tinternal.h\\\n common.h\n"
    assert B.parse_depfile(text) == [
        "/src/ks_dw.hip", "dw.hip", "/opt/my rocm/include/hip/hip runtime.h", "internal.h", "common.h"]
    assert B.parse_depfile("a.o: x\\#y.h $$z.h\n") == ["x#y.h", "$z.h"]
    assert B.parse_depfile("a.o:\n") == []
    assert B.parse_depfile("") is None and B.parse_depfile("no colon here\n") is None


def test_escaped_space_path_is_checked(tree):
    csrc, obj = tree
    (csrc / "my header.h").write_text("")
    os.utime(csrc / "my header.h", (T_NEW, T_NEW))
    (obj / "api_onp.o.d").write_text("api_onp.o: api_onp.hip \\\n  my\\ header.h\n")
    assert stale(csrc, "api_onp.hip")
    os.utime(csrc / "my header.h", (T_SRC, T_SRC))
    assert not stale(csrc, "api_onp.hip")


def test_units_are_the_api_units_and_every_kernel_set(tmp_path, monkeypatch):
    real = os.path.join(REPO, "spp-rl_amd", "csrc")
    got = [os.path.relpath(u, real) for u in B.units()]
    ks = sorted(os.path.basename(f) for f in glob.glob(os.path.join(real, "ks_*.hip")))
    api = ["api.hip", "api_comm.hip", "api_onp.hip", "api_replay.hip"]
    assert ks and got == api + ks
    assert all(os.path.exists(u) for u in B.units())
    # no other file is picked up, whatever it is called
    for f in api + ["api_old.hip", "api.hip.bak", "unity_prof.hip", "ks_x.hip", "ks_x.hip.orig", "dw.hip"]:
        (tmp_path / f).write_text("")
    monkeypatch.setattr(B, "CSRC", str(tmp_path))
    assert [os.path.basename(u) for u in B.units()] == api + ["ks_x.hip"]


def test_api_units_keep_to_their_own_kernel_files():
    """The real depfiles of the last build: the replay unit alone compiles replay.hip / stats.hip and reads nothing
    of the agent's; the RCCL unit reads no kernel file at all."""
    obj = os.path.join(REPO, "spp-rl_amd", "build")
    if not glob.glob(os.path.join(obj, "*.o.d")):
        pytest.skip("no depfiles under spp-rl_amd/build (run __graft_entry__.build())")

    def names(unit):
        with open(os.path.join(obj, unit + ".o.d")) as f:
            deps = B.parse_depfile(f.read())
        assert deps, unit
        return {os.path.basename(d) for d in deps}

    replay = names("api_replay")
    assert {"replay.hip", "stats.hip"} <= replay
    assert not replay & {"sac.hip", "ddpg.hip", "kset.h", "sgd_mlp.hip"}
    assert not names("api") & {"replay.hip", "stats.hip"}
    assert [d for d in names("api_comm") if d.endswith(".hip")] == ["api_comm.hip"]
    assert not names("api_onp") & {"replay.hip", "stats.hip"}


def test_job_count_comes_from_the_environment_and_is_capped(monkeypatch):
    monkeypatch.delenv("MAX_JOBS", raising=False)
    monkeypatch.delenv("CMAKE_BUILD_PARALLEL_LEVEL", raising=False)
    assert B._jobs(16) == 8 and B._jobs(3) == 3 and B._jobs(0) == 1
    monkeypatch.setenv("CMAKE_BUILD_PARALLEL_LEVEL", "12")
    assert B._jobs(16) == 12
    monkeypatch.setenv("MAX_JOBS", "64")
    assert B._jobs(40) == 16 and B._jobs(5) == 5
