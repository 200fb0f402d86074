"""The checks of tests/test_update_rules_cpu.py on a device arena: the rules' device forms (the
kernels of optim.hip, q8.hip, lars.hip, adamw.hip, lamb.hip, gguard.hip) behind
ParameterServer.update_range."""
import pytest

from .test_update_rules_cpu import (ELEMENTWISE, RULES, WHOLE, check_every_route_updates, check_image_of_the_caller,
                                    check_partial_range_is_refused, check_ranges_give_the_whole_rounds_bits)

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("rule", ELEMENTWISE)
def test_ranges_give_the_whole_rounds_bits(rule):
    check_ranges_give_the_whole_rounds_bits(rule, DEV)


@pytest.mark.parametrize("rule", WHOLE)
def test_partial_range_is_refused(rule):
    check_partial_range_is_refused(rule, DEV)


@pytest.mark.parametrize("rule", list(RULES))
def test_image_of_the_caller(rule):
    check_image_of_the_caller(rule, DEV)


@pytest.mark.parametrize("rule", list(RULES))
def test_every_route_updates(rule):
    check_every_route_updates(rule, DEV)
