"""The quantizer modules reach the same Function or C++ node, with the pre-op folded or materialised as before, on every
case of tests/route_cases.py: the signatures equal those recorded in tests/golden/quantizer_routes.json on the commit
before the route decision was gathered in RescalingIntQuant._route, and every route of that decision is in the table.

The table interns the signatures: {"signatures": [signature, ...], "cases": {case id: [signature index, route name of
RescalingIntQuant._route or null for the other classes]}}."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'quantizer_routes.json')


def observed():
    """-> ({case id: signature}, {case id: route name}) at this commit"""
    import route_cases
    from brevitas_amd.core.quant.int import RescalingIntQuant
    routes = {}

    def observe(cid, q):
        if type(q) is RescalingIntQuant:
            inner = q._route

            def spy(*args):
                out = inner(*args)
                routes[cid] = out[0]
                return out
            q._route = spy
    return route_cases.run(observe), routes


@pytest.mark.gpu
def test_every_case_takes_its_recorded_route():
    from brevitas_amd.core.quant.int import RescalingIntQuant
    with open(GOLDEN) as f:
        golden = json.load(f)
    table, routes = observed()
    assert sorted(table) == sorted(golden['cases']), 'the case list and the recorded table differ'
    wrong = []
    for cid, (index, route) in golden['cases'].items():
        if table[cid] != golden['signatures'][index]:
            wrong.append('%s: %s, recorded %s' % (cid, table[cid], golden['signatures'][index]))
        elif routes.get(cid) != route:
            wrong.append('%s: route %s, recorded %s' % (cid, routes.get(cid), route))
    assert not wrong, '%d cases differ:\n%s' % (len(wrong), '\n'.join(wrong[:40]))
    # the matrix misses no branch of the route decision
    recorded = {route for _, route in golden['cases'].values() if route is not None}
    assert recorded == set(RescalingIntQuant._ROUTES), recorded
