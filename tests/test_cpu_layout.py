"""The flat-buffer format, C++ against Python: every tensor offset and shape that spp-rl_amd/csrc/layout.h gives
(printed by tests/layout_dump.cpp, a stand-alone g++ program built with the address and undefined-behaviour
sanitizers and run as a child process) equals the one spprl.nets / spprl.onpolicy state, for every dimension set
the library instantiates."""
import glob
import math
import os
import re
import shutil
import subprocess

import pytest

from spprl import nets, onpolicy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "spp-rl_amd", "csrc")

# (ob, aout, ac, acm_critic) of every phase-kernel instantiation (csrc/ks_*.hip): Hopper, HalfCheetah, Ant, the
# 3-dim test set, each with the critic on the actor output or on the ACM action, and the vanilla shapes
AGENT_DIMS = [(11, 11, 3, False), (11, 11, 3, True), (17, 17, 6, False), (17, 17, 6, True),
              (111, 111, 8, False), (111, 111, 8, True), (3, 3, 1, False), (3, 3, 1, True), (17, 6, 6, False)]
# (ob, aout) of every on-policy instantiation (find_onp, csrc/api_onp.hip)
ONP_DIMS = [(17, 17), (11, 11), (17, 6), (11, 3), (3, 1)]


def cases():
    """[(maker, a, b, python layout)]"""
    out = []
    for ob, aout, ac, acmc in AGENT_DIMS:
        cin = ob + (ac if acmc else aout)
        out += [("sac_actor", ob, aout, nets.sac_actor_layout(ob, aout)),
                ("ddpg_actor", ob, aout, nets.ddpg_actor_layout(ob, aout)),
                ("critic", cin, 0, nets.critic_layout(cin)),
                ("acm", 2 * ob, ac, nets.acm_layout(2 * ob, ac)),
                ("bacm", 2 * ob, ac, nets.basic_acm_layout(2 * ob, ac))]
    for ob, aout in ONP_DIMS:
        out += [("onp_actor", ob, aout, onpolicy.actor_layout(ob, aout)),
                ("onp_critic", ob, 0, onpolicy.critic_layout(ob))]
    return out


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """{(maker, a, b): {"lead", "size", "tensors": {index: (offset, rows, cols)}, ...}} from one run of the program"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("layout") / "layout_dump")
    # (the sanitizer runtimes are linked into the program: nothing about them depends on the environment it runs in)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "layout_dump.cpp"), "-o", exe])
    args = [str(x) for mk, a, b, _ in cases() for x in (mk, a, b)]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out, cur = {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "net":
            cur = out.setdefault((w[1], int(w[2]), int(w[3])), {"lead": int(w[5]), "size": int(w[7]), "tensors": {}})
        elif w[0] == "bacm_t":
            cur["t"], cur["t1"] = int(w[1]), int(w[3])
        else:
            assert w[0] == "tensor"
            cur["tensors"][int(w[1])] = (int(w[2]), int(w[3]), int(w[4]))
    return out


def test_written_dims_are_the_instantiated_ones():
    ks = set()
    for f in glob.glob(os.path.join(CSRC, "ks_*.hip")):
        txt = open(f).read()
        for o, a, c in re.findall(r"SPP_KSET_CASE\(\w+, (\d+), (\d+), (\d+)\)", txt):
            ks |= {(int(o), int(a), int(c), False), (int(o), int(a), int(c), True)}
        for o, a, c in re.findall(r"= make_d?kset<(\d+), (\d+), (\d+), false>\(\)", txt):
            ks.add((int(o), int(a), int(c), False))
    assert ks == set(AGENT_DIMS)
    onp = re.findall(r"make_onp<(\d+), (\d+)>\(\)", open(os.path.join(CSRC, "api_onp.hip")).read())
    assert {(int(o), int(a)) for o, a in onp} == set(ONP_DIMS)


@pytest.mark.parametrize("maker", ["sac_actor", "ddpg_actor", "critic", "acm", "bacm", "onp_actor", "onp_critic"])
def test_offsets_and_shapes_match_python(dumped, maker):
    mine = [c for c in cases() if c[0] == maker]
    assert mine
    for mk, a, b, lay in mine:
        d = dumped[(mk, a, b)]
        assert d["size"] == nets.numel(lay), (mk, a, b)
        off, idx, lead = 0, 0, {}
        for name, shape in lay:
            if name.endswith(".weight") or name.endswith(".bias"):
                rows, cols = (shape[0], shape[1]) if name.endswith(".weight") else (shape[0], 0)
                assert d["tensors"][idx] == (off, rows, cols), (mk, a, b, name)
                idx += 1
            else:  # raw leading scalars: before every layer
                assert idx == 0, (mk, name)
                lead[name] = off
            off += math.prod(shape)
        assert idx == len(d["tensors"]) and d["lead"] == sum(math.prod(s) for n, s in lay if n in lead), (mk, a, b)
        if mk == "bacm":
            assert (d["t"], d["t1"]) == (lead["t"], lead["t1"])
        if mk == "onp_actor":
            assert lead == {"log_scale": 0}
