// The host checks of the stage drivers that return a code: each is what its entry runs on the HOST copy of the frame before any HIP call
// (0, or the entry's negative VVC355_*_E_*).  Library-internal, so that vvc355_picture_pass (picture.cpp) can refuse a whole picture
// before the first launch of any stage.
#pragma once
#include "../../include/vvc_mi355.h"

namespace vvc355 {

int intra_tb_check(const vvc355_intra_tb_frame *f);                     // itx.hip
int inter_tb_check(const vvc355_inter_tb_frame *f, int channels);       // itx.hip
int ts_tb_check(const vvc355_ts_tb_frame *f, int channels);             // itx.hip
int ciip_frame_check(const vvc355_ciip_frame *F, int bd);               // inter_cu.hip; bd < 0: no bit depth to check (the build entry)
int bs_rec_check(const vvc355_bs_rec_frame *f);                         // bs_rec.hip
int qp_rec_check(const vvc355_qp_rec_frame *f);                         // qp_rec.hip
int lmcs_frame_check(const vvc355_lmcs_frame *f, int bd);               // loopfilter.hip

} // namespace vvc355
