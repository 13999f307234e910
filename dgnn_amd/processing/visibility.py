"""The classical visibility votes (Labatut et al.) from the ray features of a scene: every ray votes `outside` for each cell it crosses on
its way to the sensor and `inside` for the cells just behind its surface point.  With ops.binary_graph_cut / weighted_graph_cut the votes
give a reconstruction without a network: the baseline the learned method is compared against."""
from __future__ import annotations

import numpy as np
import torch


def visibility_logits(features, infinite, infinite_vote):
    """features: the result of build_scene_features(facet_rays=True) (its "cbvf" and "cbff" columns are read), infinite [n_cells]: 1 = infinite
    cell.  -> fp32 tensor [n_cells, 2]: column 0 = cb_vertex_inside_count + cb_facet_inside_first_count (the rays that have the cell behind
    their point), column 1 the same for outside (the rays that see through the cell); infinite cells get (0, infinite_vote).  In the
    graph cut's convention column 1 is the cost of labelling the cell inside, so an infinite cell is outside for any positive vote."""
    inf = np.asarray(infinite).astype(bool).reshape(-1)
    cols = dict(features["cbvf"], **features["cbff"])
    votes = np.zeros((len(inf), 2), dtype=np.float32)
    for j, side in enumerate(("inside", "outside")):
        total = np.asarray(cols["cb_vertex_%s_count" % side]) + np.asarray(cols["cb_facet_%s_first_count" % side])
        if total.shape != inf.shape:
            raise ValueError("%d feature rows for %d cells" % (len(total), len(inf)))
        votes[:, j] = total
    votes[inf] = (0.0, float(infinite_vote))
    return torch.from_numpy(votes)
