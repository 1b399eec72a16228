// emr_fused_sancheck.cpp - the host path of smhip_emr_merge_masks under the sanitizers, on the CPU: a stand-alone program
// (its own main) on the work-group emulator's build of the library (tests/emul/smhip_emul.cpp: the same kernel bodies, the
// same host orchestration and C entry).  It runs a 5 x 131 tensor with k = 5 (the k <= 16 kernel, two groups of tasks,
// own bases, octets that are no 16-byte access) and a 257 x 9 tensor with k = 2 (the k <= 4 kernel, a short last octet,
// five blocks of the fold) and compares every output with smhip_emr_merge followed by smhip_emr_mask per entry.
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/emr_fused_sancheck.cpp \
//         -o tools/emr_fused_sancheck && tools/emr_fused_sancheck
#include "../tests/emul/smhip_emul.cpp"

#include <cstdint>

namespace {

uint32_t lcg_state = 12345u;
float draw() {                                       // uniform in [-1, 1)
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (float)(int32_t)lcg_state / 2147483648.f;
}
uint16_t bf16_of(float v) { return smhip::f_to_bf16_any(v); }

int run_case(smhip_ctx* ctx, size_t rows, size_t cols, int k, bool own_bases) {
    const size_t n = rows * cols, pb = (cols + 7) / 8;
    std::vector<std::vector<uint16_t>> ft(k, std::vector<uint16_t>(n)), base(own_bases ? k : 1, std::vector<uint16_t>(n));
    std::vector<uint16_t> base_out(n), out(n), out2(n);
    for (auto& b : base)
        for (auto& v : b) v = bf16_of(0.02f * draw());
    for (int i = 0; i < k; ++i)
        for (size_t e = 0; e < n; ++e) ft[i][e] = bf16_of(smhip::bf16_to_f(base[own_bases ? i : 0][e]) + 0.003f * draw());
    for (size_t e = 0; e < n; ++e) base_out[e] = own_bases ? bf16_of(0.02f * draw()) : base[0][e];

    smhip_emr_desc d{};
    d.k = k;
    for (int i = 0; i < k; ++i) { d.finetune[i] = ft[i].data(); d.base[i] = base[own_bases ? i : 0].data(); d.alpha[i] = 1.0; }
    d.in_dtype = SMHIP_BF16; d.base_out = own_bases ? base_out.data() : base[0].data(); d.base_out_dtype = SMHIP_BF16;
    d.n = n; d.lambda = 0.5;

    std::vector<std::vector<uint8_t>> planes(k, std::vector<uint8_t>(rows * pb, 0xa5));
    std::vector<float> scales(k, -1.f), delta(n), delta2(n);
    std::vector<uint8_t*> mptr(k);
    std::vector<float*> sptr(k);
    for (int i = 0; i < k; ++i) { mptr[i] = planes[i].data(); sptr[i] = &scales[i]; }
    smhip_emr_report rep{}, rep2{};
    std::vector<smhip_emr_mask_report> mreps(k);
    int rc = smhip_emr_merge_masks(ctx, &d, rows, cols, out.data(), delta.data(), mptr.data(), sptr.data(), &rep, mreps.data(), nullptr);
    if (rc != SMHIP_OK) { fprintf(stderr, "emr_merge_masks: rc %d: %s\n", rc, smhip_last_error(ctx)); return 1; }
    rc = smhip_emr_merge(ctx, &d, out2.data(), delta2.data(), &rep2, nullptr);
    if (rc != SMHIP_OK) { fprintf(stderr, "emr_merge: rc %d: %s\n", rc, smhip_last_error(ctx)); return 1; }
    int bad = 0;
    bad += memcmp(out.data(), out2.data(), n * 2) != 0;
    bad += memcmp(delta.data(), delta2.data(), n * 4) != 0;
    bad += memcmp(&rep, &rep2, sizeof rep) != 0;
    for (int i = 0; i < k; ++i) {
        smhip_emr_mask_desc m{};
        m.finetune = ft[i].data(); m.base = d.base[i]; m.unified = out2.data(); m.dtype = SMHIP_BF16; m.rows = rows; m.cols = cols;
        std::vector<uint8_t> plane(rows * pb, 0x5a);
        float scale = -2.f;
        smhip_emr_mask_report mr{};
        rc = smhip_emr_mask(ctx, &m, plane.data(), &scale, &mr, nullptr);
        if (rc != SMHIP_OK) { fprintf(stderr, "emr_mask: rc %d: %s\n", rc, smhip_last_error(ctx)); return 1; }
        bad += memcmp(plane.data(), planes[i].data(), plane.size()) != 0;
        bad += memcmp(&scale, &scales[i], 4) != 0;
        bad += !(mr.A == mreps[i].A && mr.B == mreps[i].B && mr.D2 == mreps[i].D2 && mr.X == mreps[i].X && mr.U2 == mreps[i].U2 &&
                 mr.c == mreps[i].c && mr.nonzero == mreps[i].nonzero && mr.resid_sq == mreps[i].resid_sq);
    }
    printf("%zu x %zu, k = %d: %s\n", rows, cols, k, bad ? "MISMATCH" : "equal to emr_merge + emr_mask");
    return bad ? 1 : 0;
}

}  // namespace

int main() {
    smhip_ctx* ctx = nullptr;
    if (smhip_create(0, &ctx) != SMHIP_OK) return 2;
    int bad = run_case(ctx, 5, 131, 5, true) + run_case(ctx, 257, 9, 2, false);
    smhip_destroy(ctx);
    return bad ? 1 : 0;
}
