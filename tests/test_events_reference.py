"""CPU: the event outputs' device rule restated (tests/events_reference.py) on a hand-made step list: two events with a pause inside the
first, a daily step between them (and one inside the second, which no forcing of the suite produces), a NaN value, PEAK with a first NaN,
slots that wrap, the event that was running at the configuration, and the refusal to overwrite an unread slot."""
import numpy as np

from events_reference import FIRST, LAST, PEAK, SUM, HostEvents

NAN = float("nan")
TEN = 1.0 / 6
# (e, t0, t1, dt hours, value of column 0, of column 1)
STEPS = [
    (0, 0, 86400, 24.0, 9.0, 9.0),                   # a dry day before everything
    (1, 86400, 90000, 1.0, 1.0, NAN),                # event 1 starts; column 1 starts with a NaN
    (1, 90000, 93600, 1.0, 0.0, 0.5),                # the pause inside it (no rain, the same id); a number beats the NaN
    (1, 93600, 94200, TEN, 0.5, NAN),                # ten minutes: 0.5 / (1/6) = 3 mm/h is the peak of column 0; a NaN is not taken
    (1, 94200, 94800, TEN, 0.25, 0.25),
    (0, 94800, 97200, 1.0, 7.0, 7.0),                # (hourly steps between the events: nothing)
    (0, 172800, 259200, 24.0, 8.0, 8.0),             # the daily step between the events
    (2, 259200, 262800, 1.0, 2.0, 4.0),              # event 2
    (2, 262800, 349200, 24.0, 12.0, 120.0),          # a daily step inside it: 120 / 24 = 5 mm/h beats 4
    (2, 349200, 352800, 1.0, 0.125, 0.125),
]
KINDS = (SUM, PEAK, FIRST, LAST)


def run(h, steps=STEPS):
    for e, t0, t1, dt, a, b in steps:
        v = np.array([a, b])
        h.add(e, t0, t1, dt, [v, v, v, v])
    return h


def test_two_events_by_hand():
    h = run(HostEvents(KINDS, 2, n_slots=4))
    assert not h.lost and (h.hdr[0] == -1).all() and (h.hdr[3] == -1).all()
    assert list(h.hdr[1]) == [1, 4, 86400, 94800, 2, 2]
    assert list(h.hdr[2]) == [2, 3, 259200, 352800, 0, 2]
    s, p, f, last = h.values[1]
    assert s[0] == 1.75 and np.isnan(s[1])                      # a NaN value stays in a sum
    assert p[0] == 0.5 / TEN and p[1] == 0.25 / TEN             # the first NaN was beaten by 0.5, then by 1.5; the later NaN was not taken
    assert f[0] == 1.0 and np.isnan(f[1]) and list(last) == [0.25, 0.25]
    s, p, f, last = h.values[2]
    assert list(s) == [14.125, 124.125] and list(p) == [2.0, 5.0] and list(f) == [2.0, 4.0] and list(last) == [0.125, 0.125]
    assert not h.values[0].any() and not h.values[3].any()      # steps of no event touch nothing


def test_the_order_of_the_additions_and_the_single_division():
    """SUM adds in the order of the steps (0.1 + 0.2 + 0.3 differs from 0.3 + 0.2 + 0.1 in the last bit); PEAK divides once."""
    vals = (0.1, 0.2, 0.3)
    h = HostEvents((SUM, PEAK), 1)
    for k, v in enumerate(vals):
        h.add(1, 600 * k, 600 * (k + 1), TEN, [np.array([v])] * 2)
    assert h.values[0, 0, 0] == (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    assert h.values[0, 1, 0] == 0.3 / TEN and 0.3 / TEN != 0.3 * 6.0
    assert list(h.hdr[0]) == [1, 3, 0, 1800, 3, 0]


def test_a_peak_that_only_sees_nan_stays_nan_and_negative_zero_is_kept():
    h = HostEvents((PEAK, SUM), 2)
    h.add(1, 0, 3600, 1.0, [np.array([NAN, -0.0])] * 2)
    h.add(1, 3600, 7200, 1.0, [np.array([NAN, -0.0])] * 2)
    assert np.isnan(h.values[0, 0, 0]) and np.signbit(h.values[0, 1, 1]) and np.signbit(h.values[0, 0, 1])


def test_slots_wrap_and_an_unread_slot_is_not_overwritten():
    steps = [(e, 3600 * e, 3600 * e + 3600, 1.0, float(e), float(e)) for e in (1, 2, 3)]
    h = run(HostEvents(KINDS, 2, n_slots=2), steps)
    assert h.lost and list(h.hdr[:, 0]) == [2, 1] and h.values[1, 0, 0] == 1.0       # event 3 found slot 1 unread: event 1 is intact
    h = HostEvents(KINDS, 2, n_slots=2)
    run(h, steps[:2])
    h.drained = 1                                                                      # the host has read event 1
    run(h, steps[2:])
    assert not h.lost and list(h.hdr[:, 0]) == [2, 3] and list(h.hdr[1]) == [3, 1, 10800, 14400, 0, 1]
    assert list(h.values[1, :, 0]) == [3.0, 3.0, 3.0, 3.0]                             # FIRST and the others start over in a reused slot


def test_the_event_running_at_the_configuration_keeps_no_start():
    h = run(HostEvents(KINDS, 2, n_slots=4, running=1, drained=0), STEPS[3:])
    assert list(h.hdr[1]) == [1, 2, -1, 94800, 2, 0] and list(h.hdr[2]) == [2, 3, 259200, 352800, 0, 2]
    assert h.values[1, 0, 0] == 0.75 and h.values[1, 2, 0] == 0.5                      # sums and FIRST from the configuration on
