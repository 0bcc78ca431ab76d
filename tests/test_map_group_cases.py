"""The cases of tests/map_group_cases.py on the serial reference alone (no GPU): they show what only a shared map shows.  A caller
cannot build the group's grid from the members' own grids: walls seen once by each of two robots are 100 only in the merged render,
and the merged box is nobody's own."""
import numpy as np

import map_group_cases as gc
import map_reference as ref

RES = gc.RES


def test_room_case_needs_the_merged_map(liw):
    assert liw.FleetGroupMap is liw.map_batch.FleetGroupMap       # the class these cases are for
    c = gc.shared_room(np.random.default_rng(0), (2, 3, 1))
    tfs_of, subs_of = c["tfs_of"], c["subs_of"]
    T_g_l = gc.compose(tfs_of, c["T_g_w"], mul=lambda A, B: gc.lie_mul(liw, A, B))
    own = [ref.render(tfs_of[b], subs_of[b], RES) for b in range(3)]
    merged = ref.render(*gc.concat(T_g_l, subs_of, [0, 1, 2]), RES)
    own100 = [o["counts"][100] for o in own]
    print("cells of value 100: per robot %s, merged %d" % (own100, merged["counts"][100]))
    # more cells are 100 in the merged render than in all members' own renders together: at least one is below 100 in every member's
    assert merged["counts"][100] > sum(own100)
    for o in own:
        assert (o["width"], o["height"], o["origin_x"], o["origin_y"]) != (merged["width"], merged["height"], merged["origin_x"], merged["origin_y"])
    assert merged["rays"] == sum(o["rays"] for o in own) == 540


def test_hand_built_cases(liw):
    assert hasattr(liw.map_batch, "GMAP_EXPORTS")
    tfs_of, subs_of = gc.one_point_same_cell()
    for b in range(2):
        assert ref.render(tfs_of[b], subs_of[b], RES)["counts"] == {-1: 0, 0: 0, 50: 1, 100: 0}
    assert ref.render(*gc.concat(tfs_of, subs_of, [0, 1]), RES)["counts"] == {-1: 0, 0: 0, 50: 0, 100: 1}
    tfs_of, subs_of = gc.one_point_disjoint()
    m = ref.render(*gc.concat(tfs_of, subs_of, [0, 1]), RES)
    assert (m["width"], m["height"]) == (49, 47) and m["counts"] == {-1: 2289, 0: 12, 50: 2, 100: 0}
