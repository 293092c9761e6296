"""CPU: the stages of K2 that are written twice -- in frame_proj_tiled_body (xmaps_k2.hpp) and in k_frame_proj_pipe
(xmaps_k2pipe.hpp), because as shared functions they moved the pipelined kernel's assembly (profiles/k2_stages_identity.md) --
still say the same thing: the in-place row-maxima pass and the 7-tap sample, compared as text once comments, spacing, the
barrier's name and the tiled body's alias of the patch buffer are taken out.  A fix made to one copy and not to the other fails here."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "x_maps_amd", "csrc")


def _stage(path, first, last):
    """the text from the line holding `first` to the line holding `last`, normalised"""
    text = open(os.path.join(CSRC, path)).read()
    a = text.index(first)
    b = text.index(last, a) + len(last)
    body = re.sub(r"//[^\n]*", "", text[a:b])
    for old, new in (("k2p_lds_barrier()", "BARRIER()"), ("__syncthreads()", "BARRIER()"), ("vmax", "tile")):
        body = body.replace(old, new)
    return re.sub(r"\s+", " ", body).strip()


def test_the_row_maxima_pass_is_the_same_text_in_both_kernels():
    first, last = "const int nseg = rows_p >> 3, tasks = cols * nseg;", "= w[j];"
    tiled, pipe = _stage("xmaps_k2.hpp", first, last), _stage("xmaps_k2pipe.hpp", first, last)
    assert "k2_rowmax8(" in tiled and tiled.count("BARRIER()") == 1 and len(tiled) > 400
    assert tiled == pipe


def test_the_seven_tap_sample_is_the_same_text_in_both_kernels():
    first, last = "for (int j = 0; j < 7; ++j) best", "rows_p]);"
    assert _stage("xmaps_k2.hpp", first, last) == _stage("xmaps_k2pipe.hpp", first, last)
