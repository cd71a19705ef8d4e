"""The matrix of tests/test_gpu_kernel_forms.py reaches every form the accumulate can take (no GPU needed: the expected forms come from the
parameters and the tiles' facts).  The GPU module asserts that each cell prints its expected forms line, so together the two fail when a
change of the dispatcher stops a cell from reaching the form it is meant to cover."""
from uvc_amd import region
from kernel_forms import ARMS, FORMS, STACK, TILES, arm_params, expected_forms, form_names, parse_forms, switches


def test_the_kernel_form_matrix_covers_every_form(oracle_lib):
    reached = {}
    for tile in TILES:
        for arm in ARMS:
            p = arm_params(region.default_params(oracle_lib, platform=ARMS[arm].get("platform", 1)), arm)
            for frag32, fam_path, splits in switches(tile):
                for split in splits:
                    for f in form_names(expected_forms(p, TILES[tile], split, frag32=frag32, fam_generic=(fam_path == "generic"))):
                        reached.setdefault(f, (tile, arm, frag32, fam_path, split))
    p = arm_params(region.default_params(oracle_lib), "sscs_table")
    for f in form_names(expected_forms(p, STACK, None)):
        reached.setdefault(f, ("amplicon_stack", "sscs_table"))
    assert len(set(FORMS)) == len(FORMS)
    missing = [f for f in FORMS if f not in reached]
    assert not missing, missing
    assert set(reached) <= set(FORMS) | {"frag_generic=sweep"}, sorted(set(reached) - set(FORMS))
    # the 32-bit bucket form without a switch forcing it
    assert expected_forms(p, STACK, None)["frag"] == "b32,wave,generic"


def test_forms_line_parses():
    err = ("[uvcgpu set_reads] family form digest\n"
           "[uvcgpu accumulate] forms prep=split p2=split,generic frag=h16,split,generic family=digest duplex=digest frag_generic=all\n"
           "[uvcgpu accumulate] forms prep=none p2=none frag=b32,wave,generic family=none duplex=none frag_generic=sweep\n")
    a, b = parse_forms(err)
    assert a == dict(prep="split", p2="split,generic", frag="h16,split,generic", family="digest", duplex="digest", frag_generic="all")
    assert form_names(b) == {"frag=b32,wave,generic", "frag_generic=sweep", "fastq_only"}
