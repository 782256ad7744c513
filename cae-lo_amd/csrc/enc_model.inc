// enc_model.inc -- the encoder's model upload: plain copies of the weights and every operand image the kernels above read; part of
// encoder.hip (included last: the builders and layout constants it uses live with their kernels).
//
// Weights and activations together: the range guard first (enc_range.hip; nothing of the context is touched when it refuses), then
// every derived operand image.  hidden: the activation of conv3d_1..3 and dense_1 (tanh | relu), code: dense_2's (tanh | linear).
CAELO_API int caelo_set_encoder_model(caelo_ctx *c, const float *w1, const float *b1, const float *w2,
                                      const float *b2, const float *w3, const float *b3, const float *wd1,
                                      const float *bd1, const float *wd2, const float *bd2, int hidden, int code) {
    CAELO_REQUIRE(c && w1 && b1 && w2 && b2 && w3 && b3 && wd1 && bd1 && wd2 && bd2, "null argument");
    CAELO_REQUIRE(hidden == CAELO_ACT_TANH || hidden == CAELO_ACT_RELU, "hidden activation: CAELO_ACT_TANH or CAELO_ACT_RELU");
    CAELO_REQUIRE(code == CAELO_ACT_TANH || code == CAELO_ACT_LINEAR, "code activation: CAELO_ACT_TANH or CAELO_ACT_LINEAR");
    {
        double bound[5];
        const int rc = caelo_host_encoder_range(w1, b1, w2, b2, w3, b3, wd1, bd1, wd2, bd2, hidden, code, bound);
        if (rc < 0) return rc;
        if (rc > 0) return CAELO_ERR_ARG;   // (caelo_last_error names the layer)
    }
    struct { float **dst; const float *src; size_t n; } plain[] = {
        {&c->enc_w1, w1, 27 * 8}, {&c->enc_b1, b1, 8},   {&c->enc_w2, w2, 27 * 8 * 16}, {&c->enc_b2, b2, 16},
        {&c->enc_w3, w3, 27 * 16 * 32}, {&c->enc_b3, b3, 32}, {&c->enc_wd2, wd2, 200 * 20}, {&c->enc_bd2, bd2, 20}};
    for (auto &p : plain) {
        if (!*p.dst) CAELO_HIP(hipMalloc(p.dst, p.n * sizeof(float)));
        CAELO_HIP(hipMemcpy(*p.dst, p.src, p.n * sizeof(float), hipMemcpyHostToDevice));
    }
    {
        // C0[pos][ch] = b2[ch] + conv2(BG)[pos][ch], BG = act(b1) in every valid 8^3 cell, zero padding outside;
        // entries 8192..8199 carry bg itself (the kernel subtracts the same float it was built from)
        float c0[512 * 16 + 8], bg[8];
        for (int ch = 0; ch < 8; ++ch) bg[ch] = enc_act_host(hidden, b1[ch]);
        for (int x = 0; x < 8; ++x) for (int y = 0; y < 8; ++y) for (int z = 0; z < 8; ++z)
            for (int o = 0; o < 16; ++o) {
                float acc = b2[o];
                for (int ka = 0; ka < 3; ++ka) for (int kb = 0; kb < 3; ++kb) for (int kc = 0; kc < 3; ++kc) {
                    const int xx = x + ka - 1, yy = y + kb - 1, zz = z + kc - 1;
                    if (xx < 0 || xx >= 8 || yy < 0 || yy >= 8 || zz < 0 || zz >= 8) continue;
                    for (int ci = 0; ci < 8; ++ci) acc += bg[ci] * w2[(((ka * 3 + kb) * 3 + kc) * 8 + ci) * 16 + o];
                }
                c0[((x * 8 + y) * 8 + z) * 16 + o] = acc;
            }
        for (int ch = 0; ch < 8; ++ch) c0[512 * 16 + ch] = bg[ch];
        // + the pooled outputs of a tile pair that sees nothing but background, per pair and lane of k_enc_stage1x (S1X_BGO_OFF floats
        // in: [16 pairs][64 lanes] float2), computed on the DEVICE with the kernel's own activation (k_enc_bgo_table)
        if (!c->enc_c0) CAELO_HIP(hipMalloc(&c->enc_c0, (S1X_BGO_OFF + 16 * 64 * 2) * sizeof(float)));
        CAELO_HIP(hipMemcpy(c->enc_c0, c0, sizeof(c0), hipMemcpyHostToDevice));
        const auto k_bgo = hidden == CAELO_ACT_RELU ? k_enc_bgo_table_relu : k_enc_bgo_table;
        k_bgo<<<16, 64>>>(c->enc_c0);
        CAELO_LAUNCH_CHECK();
        CAELO_HIP(hipDeviceSynchronize());
    }
    {
        const size_t n1 = S1X_W1F_U4, n2 = S1X_W2X_U4;
        std::vector<uint4> wxv(n1 + n2);   // (a vector: an early return of CAELO_HIP must not leak the staging buffer)
        uint4 *wx = wxv.data();
        stage1x_split_weights(w1, w2, wx, wx + n1);
        if (!c->enc_w1f) CAELO_HIP(hipMalloc(&c->enc_w1f, n1 * sizeof(uint4)));
        if (!c->enc_w2x) CAELO_HIP(hipMalloc(&c->enc_w2x, n2 * sizeof(uint4)));
        CAELO_HIP(hipMemcpy(c->enc_w1f, wx, n1 * sizeof(uint4), hipMemcpyHostToDevice));
        CAELO_HIP(hipMemcpy(c->enc_w2x, wx + n1, n2 * sizeof(uint4), hipMemcpyHostToDevice));
    }
    {
        const size_t n = (size_t)2 * C3X_NPAIR * C3X_NS * 64;
        std::vector<uint4> wxv(n);
        uint4 *wx = wxv.data();
        conv3_split_weights(w3, wx);
        if (!c->enc_w3x) CAELO_HIP(hipMalloc(&c->enc_w3x, n * sizeof(uint4)));
        CAELO_HIP(hipMemcpy(c->enc_w3x, wx, n * sizeof(uint4), hipMemcpyHostToDevice));
    }
    {
        const int rc = enc_upload_dense1(wd1, bd1, DENSE_K, &c->enc_wd1x, &c->enc_bd1);
        if (rc) return rc;
    }
    {
        const size_t n = (size_t)HEAD_WQ_FLOATS;
        std::vector<float> wqv(n);
        float *wq = wqv.data();
        head_weight_fragments(wd2, wq);
        if (!c->enc_wd2q) CAELO_HIP(hipMalloc(&c->enc_wd2q, n * sizeof(float)));
        CAELO_HIP(hipMemcpy(c->enc_wd2q, wq, n * sizeof(float), hipMemcpyHostToDevice));
    }
    c->has_enc = true;
    c->enc_hidden = hidden;
    c->enc_code = code;
    return CAELO_OK;
}

// these weights with the context's current activations (tanh / tanh until caelo_set_encoder_model says otherwise)
CAELO_API int caelo_set_encoder_weights(caelo_ctx *c, const float *w1, const float *b1, const float *w2,
                                        const float *b2, const float *w3, const float *b3, const float *wd1,
                                        const float *bd1, const float *wd2, const float *bd2) {
    CAELO_REQUIRE(c, "null argument");
    return caelo_set_encoder_model(c, w1, b1, w2, b2, w3, b3, wd1, bd1, wd2, bd2, c->enc_hidden, c->enc_code);
}

CAELO_API int caelo_get_encoder_activations(caelo_ctx *c, int32_t out[2]) {
    CAELO_REQUIRE(c && out, "null argument");
    out[0] = c->enc_hidden;
    out[1] = c->enc_code;
    return CAELO_OK;
}
