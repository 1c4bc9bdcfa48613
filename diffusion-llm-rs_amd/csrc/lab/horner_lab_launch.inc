// lab/horner_lab_launch.inc -- lab build only (-DDLLM_LAB=1): launchers of the round-3 Horner kernel, the
// 128-token Horner16 tiles (lab 323) and the lab A/B dispatch of launch_horner_gemm.
// Included by linear_horner.hip under #if DLLM_LAB; the product library compiles none of it.

namespace {

template <int MODE>
void launch_horner_t(const HornerGemmArgs &a, int y_f32, hipStream_t st, int grows = 0) {
    const int nbm = (a.M + 255) / 256, nbn = a.Npad / 256;
    const unsigned nb = static_cast<unsigned>(nbm * nbn);
    const PSampleEpi ep = a.epi ? *a.epi : PSampleEpi{};
    if (a.epi)
        wq_horner_kernel<float, 1, MODE><<<nb, 512, 0, st>>>(a.X, a.M, a.K, a.wdev, a.sz, a.hr, a.sf, a.bias,
                                                             a.epi->x_prev, a.N, a.Npad, nbm, nbn, ep, grows);
    else if (y_f32)
        wq_horner_kernel<float, 0, MODE><<<nb, 512, 0, st>>>(a.X, a.M, a.K, a.wdev, a.sz, a.hr, a.sf, a.bias,
                                                             static_cast<float *>(a.Y), a.N, a.Npad, nbm, nbn, ep,
                                                             grows);
    else
        wq_horner_kernel<__half, 0, MODE><<<nb, 512, 0, st>>>(a.X, a.M, a.K, a.wdev, a.sz, a.hr, a.sf, a.bias,
                                                              static_cast<__half *>(a.Y), a.N, a.Npad, nbm, nbn, ep,
                                                              grows);
}

int launch_horner_lab(const HornerGemmArgs &a, int y_f32, hipStream_t st) {
    if (a.lab == 49 || a.lab == 50) {   // the skewed 4-slot ring (47) with the lane swaps of make_a dropped (49:
                                        // results wrong, timing only) / with the A-fragment words read in
                                        // fragment order (50, bit-identical: the product)
        if (a.lab == 49) launch_horner16_t<kH16Ring4Skew | 32768>(a, y_f32, st);
        else launch_horner16_t<kH16Ring4SkewFrag>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab >= 46 && a.lab <= 48) {   // lab A/B (bit-identical): the 4-slot ring in lockstep (46) / with the
                                        // skew (47), the 3-slot two-barrier ring (48)
        if (a.lab == 46) launch_horner16_t<kH16Ring4>(a, y_f32, st);
        else if (a.lab == 47) launch_horner16_t<kH16Ring4Skew>(a, y_f32, st);
        else launch_horner16_t<kH16Ring3>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    // (Variants 40..45 below instantiate the 3-slot two-barrier schedule, kH16Ring3: the product kernel
    // until the 4-slot ring, lab 48 today.  The 4-slot ring excludes MODE bits 3 and 6.)
    if (a.lab == 44 || a.lab == 45) {   // lab: the 3-slot schedule without stores (44, timing only) / with the
        // 8-B register stores instead of the LDS-staged 16-B rows (45, bit-identical)
        if (a.lab == 44) launch_horner16_t<1 | 256 | 1024 | 2>(a, y_f32, st);
        else launch_horner16_t<1 | 256 | 1024 | 4096>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab >= 40 && a.lab <= 43) {   // lab ablations of the 3-slot schedule (variants 340..343; results
        // wrong, timing only): 40 no Horner rescale, 41 no rescale and the A fragments built once (no
        // dequant VALU in the loop), 42 no DMA after the prologue, 43 MFMAs + LDS reads + barriers only
        // (41 + 42, no stores)
        if (a.lab == 40) launch_horner16_t<1 | 256 | 1024 | 4>(a, y_f32, st);
        else if (a.lab == 41) launch_horner16_t<1 | 256 | 1024 | 4 | 8>(a, y_f32, st);
        else if (a.lab == 42) launch_horner16_t<1 | 256 | 1024 | 64>(a, y_f32, st);
        else launch_horner16_t<1 | 256 | 1024 | 2 | 4 | 8 | 64>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab == 26 || a.lab == 27) {   // lab A/B: the 16x16x32 kernel without the stagger (26) /
                                        // with one DMA burst per stage instead of spread pieces (27)
        if (a.lab == 26) launch_horner16_t<256 | 1024>(a, y_f32, st);
        else launch_horner16_t<1 | 1024>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab == 25) {   // lab A/B: the 16x16x32 kernel with MODE bit 11 (2 % slower on one box:
                         // profiles/r04_horner/h16_early_dequant_ab.json)
        launch_horner16_t<1 | 256 | 1024 | 2048>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab == 24) {   // lab A/B: the 16x16x32 kernel with half 1's A fragments built at substep 2
        launch_horner16_t<1 | 256>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab == 21) {   // lab A/B: the round-3 MFMA shape (32x32x16) with the product schedule
        launch_horner_t<1 | 256>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab == 19 || a.lab == 20) {   // lab ablations: the MFMA shape (MODE bit 9) in the product
        // schedule (19) and in the MFMAs-only skeleton of 14 (20)
        if (a.lab == 19) launch_horner_t<1 | 256 | 512>(a, y_f32, st);
        else launch_horner_t<3 | 4 | 8 | 16 | 64 | 512>(a, y_f32, st);
        return DLLM_OK;
    }
    if (a.lab == 17 || a.lab == 18) {   // lab ablations: 17 = 305's (no stores, rescale; one dequant and
                                        // B read) with only the weight-word DMA; 18 = 305's with the spread DMA
        if (a.lab == 17) launch_horner_t<3 | 4 | 8 | 16 | 32>(a, y_f32, st);
        else launch_horner_t<3 | 4 | 8 | 16 | 256>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab == 16) {   // lab A/B: the round-3 schedule (one DMA burst per stage, no MODE bit 8)
        launch_horner_t<1>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab == 14 || a.lab == 15) {   // lab ablations: MFMAs + barriers only (no DMA, rescale, stores;
                                        // 1 dequant / B read); 15: the DMA ring + barriers only (no MFMA)
        if (a.lab == 14) launch_horner_t<3 | 4 | 8 | 16 | 64>(a, y_f32, st);
        else launch_horner_t<3 | 4 | 8 | 16 | 128>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab >= 10 && a.lab <= 12) {   // lab A/B: XCD tile groups 4 x 8 / 8 x 4 / 16 x 2
        launch_horner_t<1 | 256>(a, y_f32, st, a.lab == 10 ? 4 : a.lab == 11 ? 8 : 16);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    if (a.lab >= 1 && a.lab <= 9) {   // lab A/B: 1 no stagger; 2.. ablations (see MODE)
        if (a.lab == 1) launch_horner_t<0>(a, y_f32, st);
        else if (a.lab == 2) launch_horner_t<3>(a, y_f32, st);
        else if (a.lab == 3) launch_horner_t<2>(a, y_f32, st);
        else if (a.lab == 4) launch_horner_t<3 | 4>(a, y_f32, st);
        else if (a.lab == 5) launch_horner_t<3 | 8>(a, y_f32, st);
        else if (a.lab == 6) launch_horner_t<3 | 16>(a, y_f32, st);
        else if (a.lab == 7) launch_horner_t<3 | 4 | 8 | 16>(a, y_f32, st);
        else if (a.lab == 8) launch_horner_t<3 | 32>(a, y_f32, st);
        else launch_horner_t<3 | 64>(a, y_f32, st);
        DLLM_LAUNCH_CHECK();
        return DLLM_OK;
    }
    return fail(DLLM_ERR_INVALID_PARAMS, "unknown Horner lab variant");
}

}  // namespace

int launch_horner_rows_gemm(const HornerGemmArgs &a, int rows, int y_f32, hipStream_t st) {
    if (rows != 128) return fail(DLLM_ERR_INVALID_PARAMS, "Horner tiles: 128 rows");
    launch_horner16_t<1 | 256, 8>(a, y_f32, st);
    DLLM_LAUNCH_CHECK();
    return DLLM_OK;
}

