// The boundary-strength and maximum-filter-length rules of one 4x4 luma unit, both edge directions: vvc_deblock_bs (vvc_filter.c:374-754) in
// gather form, on registers.  Shared AS TEXT by deblock_bs_kernel (loopfilter.hip) and bs_rec_kernel (bs_rec.hip), like itx_shape_body.inc
// and for the same reason: the including kernel keeps the instructions it had when the text stood in its body.
//
// The including scope provides
//   F                              the frame: ref_poc, lfase, lfate, n_comp, hs, vs, bs[2][3], max_len_p[2], max_len_q[2]
//   x, y                           the unit's luma position
//   curr, neigh[2]                 MvField of the unit and of its P side per direction ([0] above, [1] left)
//   t0[2][2]                       [tree][dir] the transform unit's origin across the edge
//   size_q[2], size_p[2]           the luma transform unit's size across the edge, here / on the P side
//   fq[6], fn[2][6]                pcm0, cbf0, pcm1, cbf1, cbf2, joint: here / on the P side
//   sb_p[2]                        the P side lies in a sub-block coding unit
//   my_slice, n_slice[2], tile_edge[2]
//   cb0[2], cb_size[2], sb_cu      the coding unit at the luma transform unit's origin: position, size, sub-block and not intra
//   BS_RULES_OUT(table, value)     stores the unit's entry of one output table; `dir` is in scope
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
        const int a = dir ? x : y;                              // coordinate across the edge
        // a CTB edge that must not be filtered (:498-507, :583-591)
        const bool ctb_edge_off = (!F.lfase && n_slice[dir] != my_slice) || (!F.lfate && tile_edge[dir]);
        const bool strong = curr.pred_flag == 0 || neigh[dir].pred_flag == 0 || curr.ciip_flag || neigh[dir].ciip_flag;
        // ---- luma tree
        int bs = 0, len_p = 0, len_q = 0;
        const bool has_sb = sb_cu && cb_size[dir] > 8;
        if (a == t0[0][dir]) {
            if (a > 0 && !ctb_edge_off) {
                // transform-block edge (:509-545)
                const int off_c = cb0[dir] - a;
                if (fn[dir][0] && fq[0])
                    bs = 0;
                else if (strong)
                    bs = 2;
                else if (fq[1] || fn[dir][1])
                    bs = 1;
                else if (off_c && ((off_c & 7) || !has_sb))
                    bs = 0;
                else
                    bs = bs_motion(curr, neigh[dir], (const int *)F.ref_poc + my_slice * 64, (const int *)F.ref_poc + n_slice[dir] * 64);
                // derive_max_filter_length_luma (:374-397)
                if (size_p[dir] <= 4 || size_q[dir] <= 4) {
                    len_p = len_q = 1;
                } else {
                    len_p = size_p[dir] >= 32 ? 7 : 3;
                    len_q = size_q[dir] >= 32 ? 7 : 3;
                }
                if (has_sb)
                    len_q = min(5, len_q);
                if (sb_p[dir])
                    len_p = min(5, len_p);
            }
        } else if (sb_cu && !((a - cb0[dir]) & 7)) {
            // sub-block edge inside the transform unit (:399-475), both sides in the current slice
            const int *rpl = (const int *)F.ref_poc + my_slice * 64;
            bs = bs_motion(curr, neigh[dir], rpl, rpl);
            const int i = a - t0[0][dir], tsize = size_q[dir];
            len_p = len_q = (i == 4 || i == tsize - 4) ? 1 : (i == 8 || i == tsize - 8) ? 2 : 3;
        }
        BS_RULES_OUT(F.bs[dir][0], bs);
        BS_RULES_OUT(F.max_len_p[dir], len_p);
        BS_RULES_OUT(F.max_len_q[dir], len_q);
        if (F.n_comp < 3)
            continue;
        // ---- chroma tree (:642-754): transform-block edges on the 8-sample chroma grid only
        int bs_cb = 0, bs_cr = 0;
        const int grid = (8 << (dir ? F.hs : F.vs)) - 1;
        if (a == t0[1][dir] && a > 0 && !(a & grid) && !ctb_edge_off && !(fn[dir][2] && fq[2])) {
            const int joint = fn[dir][5] | fq[5];
            bs_cb = strong ? 2 : (fn[dir][3] | fq[3] | joint) ? 1 : 0;
            bs_cr = strong ? 2 : (fn[dir][4] | fq[4] | joint) ? 1 : 0;
        }
        BS_RULES_OUT(F.bs[dir][1], bs_cb);
        BS_RULES_OUT(F.bs[dir][2], bs_cr);
    }
