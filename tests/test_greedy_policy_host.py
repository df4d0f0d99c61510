"""Greedy actions inside the policy step and the persistent rollout (pc_policy_act_greedy, pc_rollout_greedy), without a GPU: the C-ABI
surface and its argument checks, PPOConfig.eval_rollout_kernel and the two command lines' flags, and the code-object metadata of the greedy
kernel instances in the shipped library -- none of them may spill where its sampled sibling does not."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

from ppo_car_amd import _capi
from ppo_car_amd.ppo import PPOConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "ppo-car_amd", "libppocar.so")
INV, NODEV = _capi.PC_ERR_INVALID_ARG, _capi.PC_ERR_NO_DEVICE
P = 4096          # a non-NULL address: the argument checks come before any device call and never dereference it


def test_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "ppocar.h")).read()
    for name in ("pc_policy_act_greedy", "pc_rollout_greedy"):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib, name) is not None
    # the declared parameter lists: pc_policy_act's without seed / offset / offset_dev, pc_rollout_final_obs's without them
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int pc_policy_act_greedy(const pc_policy* p, const float* obs, int64_t N, const float* image, int64_t* action, float* action_f32, "
            "float* logprob, float* value, float* logits_out, void* stream);") in flat
    assert ("int pc_rollout_greedy(pc_env* e, const pc_policy* p, const float* image, int64_t T, double reward_scale, float* obs_buf, float* act_buf, "
            "float* rew_buf, float* val_buf, float* term_buf, float* trunc_buf, float* logprob_buf, float* next_obs, float* next_term, "
            "float* next_trunc, float* last_value, float* reward_sum, float* final_obs, int64_t slots, void* stream);") in flat


@pytest.fixture
def policy():
    """a handle on an impossible device: creation needs no GPU, and a call whose arguments are fine gets as far as the device check"""
    h = C.c_void_p()
    assert _capi.lib.pc_policy_create(-1, 23, 256, 9, 2, -1, C.byref(h)) == 0
    yield h
    _capi.lib.pc_policy_destroy(h)


def _act(h, obs=P, N=8, image=P, action=P, action_f32=P, logprob=P, value=P, logits=P):
    return _capi.lib.pc_policy_act_greedy(h, obs, N, image, action, action_f32, logprob, value, logits, None)


@pytest.mark.parametrize("kw", [dict(obs=None), dict(image=None), dict(action=None), dict(logprob=None), dict(value=None), dict(N=0), dict(N=-5)])
def test_policy_act_greedy_argument_checks(policy, kw):
    assert _act(policy, **kw) == INV                     # pc_policy_act's checks, before the device (-1) is looked at
    assert _act(None, **kw) == INV


def test_policy_act_greedy_null_handle_and_optional_outputs(policy):
    assert _act(None) == INV
    assert _act(policy) == NODEV                         # every argument fine: the call reaches the device check
    assert _act(policy, action_f32=None, logits=None) == NODEV


def _roll(T=8, slots=1, final_obs=None, e=None, p=None, image=P, ptrs=None):
    ptrs = [P] * 10 if ptrs is None else ptrs
    return _capi.lib.pc_rollout_greedy(e, p, image, T, 0.1, *ptrs, P, P, final_obs, slots, None)


@pytest.mark.parametrize("kw", [dict(final_obs=P, slots=0), dict(final_obs=P, T=1001, slots=1), dict(final_obs=P, T=0), dict(final_obs=P, T=-1),
                                dict(final_obs=P, slots=-1)])
def test_rollout_greedy_final_obs_checks(policy, kw):
    assert _roll(**kw) == INV                            # pc_rollout_final_obs's `slots` check, first
    assert _roll(p=policy, **kw) == INV


def test_rollout_greedy_null_handles(policy):
    assert _roll() == INV and _roll(final_obs=P, slots=1) == INV and _roll(p=policy) == INV      # (rollout_run: NULL env / policy handle)
    assert _roll(slots=0) == INV                         # final_obs NULL: `slots` is ignored -- the refusal is the NULL handles'


def test_config_validation():
    assert PPOConfig().eval_rollout_kernel == "auto"
    for ok in ("auto", "mega", "steps"):
        assert PPOConfig(eval_rollout_kernel=ok).eval_rollout_kernel == ok
    for bad in ("greedy", "", None, "MEGA"):
        with pytest.raises(ValueError, match="eval_rollout_kernel"):
            PPOConfig(eval_rollout_kernel=bad)


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags():
    train = _load("train")
    assert train.parse_args(["--run-name", "x"]).eval_rollout_kernel == "auto"
    a = train.parse_args(["--run-name", "x", "--eval-every", "1", "--eval-greedy", "--eval-rollout-kernel", "mega"])
    assert a.eval_rollout_kernel == "mega" and a.eval_greedy is True
    with pytest.raises(SystemExit):
        train.parse_args(["--run-name", "x", "--eval-rollout-kernel", "fast"])
    evaluate = _load("evaluate")
    assert evaluate.parse_args(["--checkpoint", "m.dat"]).rollout_kernel == "auto"
    b = evaluate.parse_args(["--checkpoint", "m.dat", "--envs", "64", "--greedy", "--rollout-kernel", "mega"])
    assert b.rollout_kernel == "mega" and b.greedy is True and b.envs == 64
    with pytest.raises(SystemExit):
        evaluate.parse_args(["--checkpoint", "m.dat", "--rollout-kernel", "fast"])


# ---- the greedy instances' resources, from the code object's metadata --------------------------------------------------------------------
GREEDY = re.compile(r"^(_Z\d+(?:policy_kernel|rollout_kernel|rollout_small_kernel)I(?:L[ib]\d+E)+)Lb1E(Ev.*)$")


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel symbol: {"vgpr_spill_count": n, "private_segment_fixed_size": n, ...}} of the gfx950 code object inside libppocar.so"""
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not found under {LLVM}")
    if not os.path.exists(LIB):
        pytest.skip("libppocar.so is not built")
    d = tmp_path_factory.mktemp("greedy_meta")
    fat, co = str(d / "fat.bin"), str(d / "co.o")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", LIB, str(d / "unused.so")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}", "--unbundle"])
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    shutil.rmtree(d, ignore_errors=True)
    out, cur = {}, None
    for line in notes.split("\n"):
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)       # an entry of amdhsa.kernels opens with "  - .key:", its keys sit at indent 4
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        key, val = m.group(2), m.group(3).strip().strip("'\"")
        if cur is not None and key == "symbol":
            out[val[:-3] if val.endswith(".kd") else val] = cur
        elif cur is not None and re.fullmatch(r"-?\d+", val):
            cur[key] = int(val)
    assert len(out) > 100
    return out


def test_greedy_instances_spill_no_more_than_their_sampled_siblings(metadata):
    greedy = {n: GREEDY.match(n) for n in metadata if GREEDY.match(n)}
    families = {fam: sum(n.startswith(f"_Z{len(fam)}{fam}I") for n in greedy) for fam in ("policy_kernel", "rollout_kernel", "rollout_small_kernel")}
    # every form of the policy step (3 K widths x split x 3 precisions); the big form's 8 single-track modes + the two 16-envs-per-wave
    # layouts; the small form's 6
    assert families == {"policy_kernel": 18, "rollout_kernel": 8 + 2, "rollout_small_kernel": 6}, families
    for name, m in greedy.items():
        sibling = m.group(1) + "Lb0E" + m.group(2)
        assert sibling in metadata, (name, "has no sampled sibling")
        g, s = metadata[name], metadata[sibling]
        for key in ("vgpr_spill_count", "private_segment_fixed_size"):
            assert g[key] <= s[key], (name, key, g[key], s[key])
