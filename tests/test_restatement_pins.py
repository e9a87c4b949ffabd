"""The CPU restatements (tests/*_helpers.py: MipRef, IsoRef, ClipRef, ShadowRef, LightRef, SlabRef, BackdropRef) still return what they
returned at the commit tests/golden/restatement_pins.json names: every frame, depth layer, light grid, integral table, segment list and
counter that oracle/gen_restatement_pins.py walks, under one FNV-1a32 per entry.  The fixture was taken while each entry point had a C
text of its own (clip_ref.c, shadow_ref.c, light_ref.c, slab_ref.c, backdrop_ref.c, iso_ref.c, mip_ref.c); tests/feature_ref.c states
them once, and this test is what holds that single text to the seven it replaced — the ties between two wrappers of one ray in the
*_model.py tests no longer compare two texts."""
import importlib.util
import json
import os

import feature_random as fr
from helpers import GOLDEN_DIR, ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("gen_restatement_pins", os.path.join(ROOT, "oracle", "gen_restatement_pins.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_every_pinned_hash_is_reproduced(vr, golden, oracle):
    """Every entry of the fixture — one entry point on one case, one FNV-1a32 over the hashes of all its arrays and its counters
    (gen_restatement_pins.fold) — and the list that is walked and the list that was recorded have the same entries.  A failure names the
    entry and prints the hash of each of its outputs, to be set beside the same print on the tree the fixture names.  The random and
    edge frames are those of the committed seed: under another VR_TEST_SEED they are other frames and are not compared."""
    gen = _generator()
    with open(os.path.join(GOLDEN_DIR, "restatement_pins.json")) as f:
        pinned = json.load(f)
    want = {(entry, case): h for group in pinned["pins"] for case, entries in group.items() for entry, h in entries.items()}
    assert len(want) > 700
    seeded = fr.SEED == pinned["seed"]
    source = gen.pins(vr, golden, oracle) if seeded else list(gen.golden_pins(vr, golden)) + list(gen.remaining_pins(vr, golden, oracle))
    seen = 0
    for entry, case, out in source:
        digests = gen.digest(out)
        assert gen.fold(digests) == want[(entry, case)], (entry, case, digests)
        seen += 1
    assert seen == len(want) - (0 if seeded else sum(1 for entry, _ in want if entry == "feature_random")), (seen, len(want))
    print(f"{seen} entries reproduced from commit {pinned['commit'][:7]}")
