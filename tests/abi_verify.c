/* A strict C99 caller of the verifier entry points of g16_mi355x.h (host forms: no GPU needed).  BLS12-381:
 * e(g1, g2) from g16_host_pairing is not 1, e(g1, g2) * e(-g1, g2) is 1, and a zero-input key with a proof of
 * points that are off the curve gives verdict 2; a wrong input count is G16_ERR_MALFORMED_VK. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "g16_mi355x.h"

/* BLS12-381 generators in arkworks' Montgomery form, computed here from canonical limbs through g16_host_field_op */
static const uint64_t G1X[6] = {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull, 0xc3688c4f9774b905ull,
                                0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull};
static const uint64_t G1Y[6] = {0x0caa232946c5e7e1ull, 0xd03cc744a2888ae4ull, 0x00db18cb2c04b3edull, 0xfcf5e095d5d00af6ull,
                                0xa09e30ed741d8ae4ull, 0x08b3f481e3aaa0f1ull};
static const uint64_t G2[4][6] = {
    {0xd48056c8c121bdb8ull, 0x0bac0326a805bbefull, 0xb4510b647ae3d177ull, 0xc6e47ad4fa403b02ull, 0x260805272dc51051ull, 0x024aa2b2f08f0a91ull},
    {0xe5ac7d055d042b7eull, 0x334cf11213945d57ull, 0xb5da61bbdc7f5049ull, 0x596bd0d09920b61aull, 0x7dacd3a088274f65ull, 0x13e02b6052719f60ull},
    {0xe193548608b82801ull, 0x923ac9cc3baca289ull, 0x6d429a695160d12cull, 0xadfd9baa8cbdd3a7ull, 0x8cc9cdc6da2e351aull, 0x0ce5d527727d6e11ull},
    {0xaaa9075ff05f79beull, 0x3f370d275cec1da1ull, 0x267492ab572e99abull, 0xcb3e287e85a763afull, 0x32acd2b02bc28b99ull, 0x0606c4a02ea734ccull}};

static const uint64_t R_MINUS_1[4] = {0xffffffff00000000ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};

static int to_mont(const uint64_t* canon, uint64_t* out) { return g16_host_field_op(G16_BLS12_381, 1, 5, canon, NULL, out); }

int main(void) {
    uint64_t g1[12], g2[24], pairs1[24], pairs2[48], gt[72], one[72];
    int i, rc;
    uint8_t verdict = 9;
    g16_vk_view vk;
    uint64_t proof[48];
    if (to_mont(G1X, g1) || to_mont(G1Y, g1 + 6)) { printf("to_mont failed\n"); return 1; }
    for (i = 0; i < 4; ++i)
        if (to_mont(G2[i], g2 + 6 * i)) { printf("to_mont failed\n"); return 1; }
    rc = g16_host_pairing(G16_BLS12_381, g1, g2, 1, gt);
    if (rc) { printf("g16_host_pairing: %s\n", g16_strerror(rc)); return 1; }
    rc = g16_host_pairing(G16_BLS12_381, g1, g2, 0, one);   /* empty product: 1 */
    if (rc || memcmp(gt, one, sizeof gt) == 0) { printf("e(g1, g2) is 1\n"); return 1; }
    memcpy(pairs1, g1, sizeof g1);
    memcpy(pairs1 + 12, g1, sizeof g1);
    rc = g16_host_group_op(G16_BLS12_381, 0, 1, g1, R_MINUS_1, pairs1 + 12);   /* (r - 1) g1 = -g1 */
    if (rc) { printf("g16_host_group_op: %s\n", g16_strerror(rc)); return 1; }
    memcpy(pairs2, g2, sizeof g2);
    memcpy(pairs2 + 24, g2, sizeof g2);
    rc = g16_host_pairing(G16_BLS12_381, pairs1, pairs2, 2, gt);
    if (rc || memcmp(gt, one, sizeof gt) != 0) { printf("e(g1, g2) e(-g1, g2) != 1\n"); return 1; }
    vk.alpha_g1 = g1; vk.beta_g2 = g2; vk.gamma_g2 = g2; vk.delta_g2 = g2; vk.gamma_abc_g1 = g1; vk.n_gamma_abc = 1;
    for (i = 0; i < 48; ++i) proof[i] = 1; /* not a point */
    rc = g16_host_verify(G16_BLS12_381, &vk, proof, NULL, 0, &verdict);
    if (rc || verdict != 2) { printf("off-curve proof: rc %d verdict %d\n", rc, verdict); return 1; }
    rc = g16_host_verify(G16_BLS12_381, &vk, proof, g1, 1, &verdict);
    if (rc != G16_ERR_MALFORMED_VK) { printf("wrong input count: rc %d\n", rc); return 1; }
    if (g16_struct_size(G16_STRUCT_VK_VIEW) != sizeof(g16_vk_view)) { printf("g16_vk_view size\n"); return 1; }
    printf("abi_verify ok\n");
    return 0;
}
