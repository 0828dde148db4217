"""The host side the three training families share (buzzdetect_amd/csrc/headtrain_host.h: the lone trainer, the bank of heads,
the bank of stacks): the header is built and hashed, the three .hip files include it and define none of its routines again, the
layer-by-layer route of Dense stacks (headtrain_stack.h) is the one copy of its kernels and launches for the lone trainer and
the bank of stacks, the bias-corrected Adam rate is written once, and every refusal gives the return code and the words
recorded before the host side was shared (tests/golden/train_refusals.json, tools/record_train_refusals.py).  No GPU needed."""
import ctypes as C
import json
import os
import re

import pytest

from buzzdetect_amd import _lib, build
from tools import record_train_refusals as R

SOURCES = ("headtrain.hip", "headbank.hip", "stackbank.hip")
# what headtrain_host.h defines for all three: functions, then types, then the rest
SHARED_FUNCTIONS = ("check_training_setup", "check_stack", "select_device", "check_member", "check_batch", "check_row_weights",
                    "adam_rate", "members_from", "set_learning_rate", "set_weight_decay", "set_frozen", "snapshot_member",
                    "restore_member", "loss_inv", "loss_scale", "slices_of", "up64", "stack_layout", "upload_stack", "copy_stack",
                    "read_stack_pair", "mean_losses", "workspace_floats", "workspace_fill", "workspace_read", "destroy", "enter",
                    "enter_and_wait")
FORMER_COPIES = ("check_weights", "members_of", "inv_of", "scale_of", "width_of")      # the names the copies had
SHARED_TYPES = ("Members", "MemberState", "TrainHandle", "StackLayer", "StackLayout")
STACK_HEADER = "headtrain_stack.h"                              # the layer-by-layer route headtrain.hip and stackbank.hip run
STACK_SOURCES = ("headtrain.hip", "stackbank.hip")
STACK_KERNELS = ("stack_forward_kernel", "stack_loss_rows_kernel", "stack_loss_sum_kernel", "stack_weight_grad_kernel",
                 "stack_input_grad_kernel", "stack_apply_kernel")


def read(name):
    with open(os.path.join(build.CSRC, name)) as f:
        return f.read()


def read_with_stack_header(name):
    """The file, and behind it the stack header if the file includes it: where a call may have moved to."""
    text = read(name)
    return text + read(STACK_HEADER) if '#include "' + STACK_HEADER + '"' in text else text


def defines_function(name, text):
    """A definition: a return type, the bare name, a parameter list, a brace - not a call, not an entry point bd_*_<name>."""
    return re.search(r"^[ \t]*(?:[\w:<>]+[\s*&]+)+" + name + r"\s*\([^;{}]*\)\s*(?:const\s*)?\{", text, re.M)


def test_the_host_header_is_built_hashed_and_included():
    assert "headtrain_host.h" in build.HEADERS and "headtrain_device.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "headtrain_host.h"))
    for source in SOURCES:
        assert source in build.SOURCES
        text = read(source)
        assert '#include "headtrain_host.h"' in text, source
        assert text.index('#include "headtrain_device.h"') < text.index('#include "headtrain_host.h"'), source
    assert STACK_HEADER in build.HEADERS and os.path.exists(os.path.join(build.CSRC, STACK_HEADER))
    for source in SOURCES:
        text = read(source)
        assert ('#include "' + STACK_HEADER + '"' in text) == (source in STACK_SOURCES), source
        if source in STACK_SOURCES:
            assert text.index('#include "headtrain_host.h"') < text.index('#include "' + STACK_HEADER + '"'), source


def test_the_layer_by_layer_kernels_are_written_once():
    kernels = {source: re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", read(source))
               for source in STACK_SOURCES + (STACK_HEADER,)}
    assert kernels["headtrain.hip"] == ["fused_step_kernel"] and read("headtrain.hip").count("__global__") == 1
    assert kernels["stackbank.hip"] == [] and "__global__" not in read("stackbank.hip")
    assert sorted(kernels[STACK_HEADER]) == sorted(STACK_KERNELS)
    for source in STACK_SOURCES:
        assert "hipLaunchKernelGGL(" not in read(source).replace("hipLaunchKernelGGL(bd::fused_step_kernel<", ""), source
        assert re.search(r"\bStackRun run_of\(", read(source)), source


def test_the_host_header_holds_host_code_only():
    header = read("headtrain_host.h")
    assert "__global__" not in header and "__device__" not in header
    assert "hipLaunchKernelGGL" not in header and "<<<" not in header


def test_no_training_file_defines_a_shared_routine_again():
    header = read("headtrain_host.h")
    for name in SHARED_FUNCTIONS:
        assert defines_function(name, header), f"headtrain_host.h does not define {name}"
    for name in SHARED_TYPES:
        assert re.search(r"\bstruct " + name + r"\b[^;]*\{", header), name
    # fail and the HIP-check macro are the whole library's one copy (bd_error.h), which the header includes and does not repeat
    errors = read("bd_error.h")
    assert '#include "bd_error.h"' in header and "bd_error.h" in build.HEADERS
    assert defines_function("fail", errors) and not defines_function("fail", header)
    assert len(re.findall(r"#define \w+_HIP\(", errors)) == 1 and not re.search(r"#define \w+_HIP\(", header)
    assert "kMembersPerLaunch =" in header and "set_error(const" not in header
    for source in SOURCES:
        text = read(source)
        for name in SHARED_FUNCTIONS + ("fail",) + FORMER_COPIES:
            assert not defines_function(name, text), f"{source} defines {name}"
        for name in SHARED_TYPES + ("Layer",):
            assert not re.search(r"\bstruct " + name + r"\b[^;]*\{", text), f"{source} defines {name}"
        assert not re.search(r"#define \w+_HIP\(", text), f"{source} has a HIP-check macro of its own"
        assert "kMembersPerLaunch =" not in text and "set_error(const" not in text, source
        assert re.search(r"^struct bd_\w+_s : bd::TrainHandle \{", text, re.M), f"{source}'s handle is no TrainHandle"
    assert "fill_kernel" not in read("headtrain.hip")       # the workspace is filled the banks' way
    # the calls the three families have in common go through the one copy
    for source in SOURCES:
        text = read_with_stack_header(source)
        for name in ("check_training_setup", "select_device", "check_batch", "check_row_weights", "enter", "set_learning_rate",
                     "set_weight_decay", "mean_losses", "workspace_floats", "workspace_fill", "workspace_read", "destroy", "loss_inv",
                     "loss_scale", "slices_of"):
            assert re.search(r"\b" + name + r"\(", text), f"{source} does not call {name}"
    for source in ("headbank.hip", "stackbank.hip"):
        text = read_with_stack_header(source)
        for name in ("launch_args", "members_from", "set_frozen", "snapshot_member", "restore_member", "check_member"):
            assert re.search(r"\b" + name + r"(<\w+>)?\(", text), f"{source} does not call {name}"      # (<capacity>: of a launch)
    for source in STACK_SOURCES:
        text = read_with_stack_header(source)
        for name in ("check_stack", "stack_layout", "upload_stack", "copy_stack", "read_stack_pair"):
            assert re.search(r"\b" + name + r"\(", text), f"{source} does not call {name}"


def test_the_adam_rate_is_written_once():
    holders = [name for name in sorted(os.listdir(build.CSRC)) if name.endswith((".hip", ".h"))
               and re.search(r"std::pow\([^;]*beta_2", read(name))]
    assert holders == ["headtrain_host.h"]
    assert [name for name in sorted(os.listdir(build.CSRC)) if name.endswith((".hip", ".h")) and "std::pow(" in read(name)] == holders
    header = read("headtrain_host.h")
    assert header.count("std::pow(") == 2                    # beta_2^t and beta_1^t of the one expression
    # the trainer's update and a bank's launch arguments are built from it by one routine
    assert header.count("adam_rate(") == 2 and len(re.findall(r"\bupdate_of\(", header)) == 2
    # (the trainer's update is the launch arguments of its one member: launch_args, which calls update_of)
    assert re.search(r"\blaunch_args<1>\(", read("headtrain.hip")) and re.search(r"= update_of\(", header)
    for source in SOURCES + (STACK_HEADER,):
        assert "adam_rate(" not in read(source) and "std::sqrt(" not in read(source), source


# ---------------------------------------------------------------------------------------------------- the refusals' words
with open(R.GOLDEN) as _f:
    RECORDED = json.load(_f)


def no_device_visible():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_the_recorded_cases_are_the_cases():
    table, _ = R.cases(_lib.load())
    assert sorted(table) == sorted(RECORDED) and len(RECORDED) > 120
    for family, prototypes in (("bd_trainer_", _lib.TRAIN_PROTOTYPES), ("bd_bank_", _lib.BANK_PROTOTYPES),
                               ("bd_stackbank_", _lib.STACKBANK_PROTOTYPES)):
        entry_points = {n for n in prototypes if n.startswith(family)} - {family + "destroy", family + "abi_version"}
        assert {n + ": null" for n in entry_points} <= set(RECORDED), family       # every entry point with a null handle
        assert RECORDED[family + "create" + R.NEEDS_NO_DEVICE][0] == -2            # BD_ENODEVICE, recorded without a device
    assert all(rc in (-1, -4) for name, (rc, _) in RECORDED.items() if not name.endswith(R.NEEDS_NO_DEVICE))


@pytest.mark.parametrize("family", ("bd_trainer_", "bd_bank_", "bd_stackbank_"))
def test_refusals_have_the_recorded_code_and_words(family):
    lib = _lib.load()
    table, handle = R.cases(lib)
    device = not no_device_visible()
    compared = 0
    for name in sorted(table):
        if not name.startswith(family) or (device and name.endswith(R.NEEDS_NO_DEVICE)):
            continue
        rc = int(table[name]())
        message = lib.bd_last_error()
        assert handle.value is None, name
        assert [rc, message] == [RECORDED[name][0], RECORDED[name][1].encode()], name
        compared += 1
    assert compared >= 35
    assert getattr(lib, family + "destroy")(None) == 0      # like free(NULL)
