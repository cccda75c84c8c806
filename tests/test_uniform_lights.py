"""What the scalar path for one-record light lists rests on (path_shade; csrc/pt_device.hpp pick_index): the uniform pick over
a list of ONE record, min(uint32(int32(u * float32(1))), 0), is 0 for every draw u the sampler can return and for the ends of
its range, so the record a lane picks does not depend on the lane."""
import numpy as np

F = np.float32


def pick_index(u, count):
    """pick_index of pt_device.hpp in numpy's float32 and integer arithmetic"""
    a = np.uint32(np.int32(F(u) * F(count)))
    b = np.uint32(count - 1)
    return min(a, b)


def test_the_pick_over_one_record_is_zero():
    draws = [F(0.0), np.nextafter(F(0.0), F(1.0)), F(0.5), np.nextafter(F(1.0), F(0.0)), F(1.0)]
    assert draws[1] > 0 and draws[3] < 1
    for u in draws:
        assert pick_index(u, 1) == 0, u


def test_the_pick_over_two_records_depends_on_the_draw():
    """the same arithmetic does tell two records apart: the scalar path is for a count of one only"""
    assert pick_index(F(0.25), 2) == 0 and pick_index(F(0.75), 2) == 1 and pick_index(F(1.0), 2) == 1
