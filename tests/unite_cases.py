"""Scenes for the tile union (mrcnn_unite_tiles / mrcnn_unite_tiles_host), shared by tests/test_unite_host.py and
tests/test_gpu_unite.py.  A scene is tiles_cases' dict; `unite` (optional) maps (metric, link_threshold) to what must come out per
image: a list of components in output order, each dict(members=[k, ...] in the order, area=, bbox=(x, y, w, h)[, rle=[...]]).

The hand-derived scenes use windows of the model's size (the letterbox is the identity, boxes come out exactly) and "full" masks (the
plane is the box), so every number below can be checked by hand: areas are columns x rows."""
import tiles_cases as TC

ROWS = 4


def k(t, i):
    return t * ROWS + i


def _hand():
    two = [[0, 0, 0, 128, 128], [0, 0, 96, 128, 128]]            # two windows of a 128 x 224 image; R = columns 96..127
    wide = [(128, 224)]
    comp = lambda members, area, bbox, **kw: dict(members=members, area=area, bbox=bbox, **kw)
    out = []

    def add(name, sizes, tiles, entries, unite):
        sc = TC.scene(name, sizes, tiles, ROWS, entries, metric="iou", match_threshold=0.5)
        sc["unite"] = unite
        out.append(sc)
    # full-frame columns 60..127 and 96..159: inside R both planes are columns 96..127 — IoU_R = 1
    halves = lambda c0, c1, s0, s1: [(0, 0, (30, 60, 70, 128), c0, s0, "full"), (1, 0, (30, 0, 70, 64), c1, s1, "full")]
    one = [comp([k(0, 0), k(1, 0)], 4000, (60, 30, 100, 40))]
    add("cut_in_two", wide, two, halves(2, 2, 0.9, 0.8), {("iou", 0.5): [one], ("ios", 0.5): [one], ("iou", 1.0): [one]})
    # columns 60..127 and 112..159: in R 32 columns against 16 of them — IoU_R = 16/32 = 0.5 exactly, IoS_R = 1
    parts = [comp([k(0, 0)], 2720, (60, 30, 68, 40)), comp([k(1, 0)], 1920, (112, 30, 48, 40))]
    add("exactly_the_threshold", wide, two, [(0, 0, (30, 60, 70, 128), 2, 0.9, "full"), (1, 0, (30, 16, 70, 64), 2, 0.8, "full")],
        {("iou", 0.5): [one], ("iou", 0.75): [parts], ("ios", 0.75): [one]})
    # columns 60..109 and 116..155 never meet
    add("neighbours", wide, two, [(0, 0, (30, 60, 70, 110), 2, 0.9, "full"), (1, 0, (30, 20, 70, 60), 2, 0.8, "full")],
        {("iou", 0.5): [[comp([k(0, 0)], 2000, (60, 30, 50, 40)), comp([k(1, 0)], 1600, (116, 30, 40, 40))]]})
    # boxes of the plane's full height: the runs cross columns in the inputs, in the clipped areas and in the union
    add("full_height", wide, two, [(0, 0, (0, 60, 128, 128), 2, 0.9, "full"), (1, 0, (0, 0, 128, 64), 2, 0.8, "full")],
        {("iou", 0.5): [[comp([k(0, 0), k(1, 0)], 12800, (60, 0, 100, 128), rle=[7680, 12800, 8192])]]})
    # the whole object (columns 60..119) and its cut copy (96..119) with the higher score
    add("whole_and_cut", wide, two, [(0, 0, (30, 60, 70, 120), 2, 0.9, "full"), (1, 0, (30, 0, 70, 24), 2, 0.95, "full")],
        {("iou", 0.5): [[comp([k(1, 0), k(0, 0)], 2400, (60, 30, 60, 40))]]})
    apart = [comp([k(0, 0)], 2720, (60, 30, 68, 40)), comp([k(1, 0)], 2560, (96, 30, 64, 40))]
    add("classes_differ", wide, two, halves(2, 3, 0.9, 0.8), {("iou", 0.5): [apart], ("ios", 0.25): [apart]})
    add("same_tile", wide, two, [(0, 0, (30, 60, 70, 128), 2, 0.9, "full"), (0, 1, (30, 96, 70, 128), 2, 0.8, "full")],
        {("iou", 0.5): [[comp([k(0, 0)], 2720, (60, 30, 68, 40)), comp([k(0, 1)], 1280, (96, 30, 32, 40))]]})
    add("score_tie", wide, two, halves(2, 2, 0.8, 0.8), {("iou", 0.5): [one]})
    # three windows of a 128 x 288 image at x0 = 0, 80, 160: windows 0 and 2 share nothing, the object crosses all three
    three = [[0, 0, 0, 128, 128], [0, 0, 80, 128, 128], [0, 0, 160, 128, 128]]
    add("chain", [(128, 288)], three, [(0, 0, (30, 20, 70, 128), 2, 0.7, "full"), (1, 0, (30, 0, 70, 128), 2, 0.9, "full"),
                                       (2, 0, (30, 0, 70, 110), 2, 0.8, "full")],
        {("iou", 0.5): [[comp([k(1, 0), k(2, 0), k(0, 0)], 10000, (20, 30, 250, 40))]]})
    return out


SEEDED = ("tiles_larger_than_the_model", "tiles_smaller_than_the_model", "inward_shifted_edge_tiles", "two_images", "max_out_below_kept")


def scenes():
    """The hand-derived scenes, then tiles_cases' seeded `_objects` scenes (larger and smaller windows, inward-shifted edge tiles, two
    images, max_out below the number of components): blob and disk masks cut at window edges — holes, islands, abutting runs."""
    seeded = [dict(sc, unite={}) for sc in TC.scenes() if sc["name"] in SEEDED]
    assert len(seeded) == len(SEEDED)
    return _hand() + seeded


def configs(sc):
    """(metric, link_threshold, max_out) to run a scene with: what it expects, both metrics, a strict and a lax threshold, a small cap."""
    base = [("iou", 0.5, sc["max_out"]), ("ios", 0.5, sc["max_out"]), ("iou", 0.9, sc["max_out"]), ("ios", 0.2, 2), ("iou", 0.3, 1)]
    return list(dict.fromkeys([(m, t, sc["max_out"]) for (m, t) in sc["unite"]] + base))
