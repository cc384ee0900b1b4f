"""Seeded random-shape sweeps of the ResNet entry points, of one FPN level (wino_fpn_level_hw: every form of its
lateral 1x1 and of its 3x3), of the grouped 3x3 layer and the two ResNeXt blocks (every one
of the kernel's twelve instantiations, named by wino_conv3x3_grouped_plan) and of the segmentation path -- the dilated 3x3 layer, the
dilated bottleneck blocks, the concat projection, ASPP and the bilinear resize -- (tests/shape_sweeps.py: shapes from the whole legal envelope
of winograd_mi355x.h, every forced form the planner takes, the automatic ones): each case against an fp64 reference
computed on the CPU (tests/sweep_cases.py: the case runners) from the raw torch-layout weights and unfolded BN vectors, into NaN-filled outputs and
workspaces, with NaN in every ring the contract says is not read, negative BN scales on a third of the channels, and
post-ReLU-like (non-negative) inputs in part of the cases.  Every launch runs twice and must repeat bit for bit; no
stream-K ticket may stay held.  tests/test_shape_sweeps_host.py checks on the host that every case is legal and that
the draws reach their corners.

Every tensor a launch sees lies on the guarded arena of tests/guarded.py: inputs (the packed filters included) between
NaN guards, outputs and workspaces of exactly the queried size between sentinel guards.  Every case launches at both
placements, 256-byte aligned and 16 mod 256 (the weakest pointer the header accepts), against the one fp64 reference,
and ends each in arena.check: no guard touched, no read-only operand written.  No case may be left out: each test
counts its checks.  The pack entry points write through out= into arena outputs of exactly the queried count, and their
consumers read the packed tensor from a guarded address."""
import pytest

import sweep_cases as SC
from gpu_support import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def test_residual_3x3_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("conv3x3_bn_add_relu", SC.residual_case, pkg, knobs, torch_dev, 100)


def test_basic_block_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("basic_block", SC.basic_block_case, pkg, knobs, torch_dev, 200)


def test_conv3x3_s2_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("conv3x3_s2_bn_relu", SC.s2_case, pkg, knobs, torch_dev, 300)


def test_conv3x3_s2_proj_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("conv3x3_s2_proj", SC.s2_proj_case, pkg, knobs, torch_dev, 400)


def test_basic_block_s2_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("basic_block_s2", SC.basic_block_s2_case, pkg, knobs, torch_dev, 500)


def test_proj_block_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("proj_block", SC.proj_case, pkg, knobs, torch_dev, 600)


def test_proj_block_v15_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("proj_block_v15", SC.v15_case, pkg, knobs, torch_dev, 700)


def test_stem_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("stem", SC.stem_case, pkg, knobs, torch_dev, 800)


def test_head_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("avgpool_fc", SC.head_case, pkg, knobs, torch_dev, 900)


def test_dilated_3x3_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("conv3x3_dilated_bn_relu", SC.dilated_case, pkg, knobs, torch_dev, SC.SEEDS["conv3x3_dilated_bn_relu"])


def test_dilated_block_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("dilated_block", SC.dilated_block_case, pkg, knobs, torch_dev, SC.SEEDS["dilated_block"])


def test_conv1x1_cat_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("conv1x1_cat_bn", SC.cat_case, pkg, knobs, torch_dev, SC.SEEDS["conv1x1_cat_bn"])


def test_aspp_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("aspp", SC.aspp_case, pkg, knobs, torch_dev, SC.SEEDS["aspp"])


def test_resize_bilinear_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("resize_bilinear", SC.resize_case, pkg, knobs, torch_dev, SC.SEEDS["resize_bilinear"])


def test_grouped_3x3_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("conv3x3_grouped_bn_relu", SC.grouped_case, pkg, knobs, torch_dev, SC.SEEDS["conv3x3_grouped_bn_relu"])


def test_grouped_block_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("grouped_block", SC.grouped_block_case, pkg, knobs, torch_dev, SC.SEEDS["grouped_block"])


def test_fpn_level_sweep(pkg, knobs, torch_dev):
    SC.run_sweep("fpn_level", SC.fpn_level_case, pkg, knobs, torch_dev, SC.SEEDS["fpn_level"])
