"""The reference side of tests/test_gpu_nonfinite.py, without a GPU: every dependency set comes from the fp64 reference alone, is not
empty, and covers less than half of an output that the node computes row-, window- or column-locally; the fp16 overflow cases overflow
and leave at most 1 % of a tensor within 10 % of 65504."""
import pytest
import torch

import test_gpu_nonfinite as NF


@pytest.mark.parametrize("case", NF.ALL_CASES, ids=lambda c: c.key)
def test_reference_masks_are_not_vacuous_and_local(case):
    n = 0
    for value in (NF.NAN, NF.INF):
        for p in case.poisons():
            masks = case.masks(p, value)
            NF.guard_masks(case, p, masks)
            clean = case.inputs()[p.name]
            assert torch.isfinite(clean.float()).all() and clean[p.idx] != 0
            n += 1
    assert n >= 4


@pytest.mark.parametrize("kind", list(NF.OVERFLOW))
def test_overflow_references_meet_the_exclusion_cap(kind):
    _, refs = NF.overflow_reference(kind)
    for name, ref in refs.items():
        expect, cmp_ = NF.overflow_sets(ref)
        assert (~cmp_).float().mean().item() <= 0.01, name
        assert expect.any() and not expect.all(), name
