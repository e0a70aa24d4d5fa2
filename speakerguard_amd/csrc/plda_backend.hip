// Host half of the PLDA back end that xv_plda and iv_plda share (PldaBackend, sg_internal.h): what the load derives and uploads,
// and the enrolled table's replacement.  The scoring itself: plda_device.h.
#include <cmath>

#include "sg_internal.h"

namespace sg {

int plda_backend_load(sg_ctx* ctx, std::vector<void*>& pool, PldaBackend* be, const float* plda_mean, const float* plda_psi,
                      const float* enroll, int D, int S, float threshold) {
    double ldg = 0.0, ldw = 0.0;
    for (int d = 0; d < D; ++d) {
        const double psi = plda_psi[d];
        ldg += std::log(1.0 + psi / (psi + 1.0));
        ldw += std::log(psi + 1.0);
    }
    int rc = SG_OK;
    rc |= dev_upload(ctx, pool, &be->plda_mean, std::vector<float>(plda_mean, plda_mean + D));
    rc |= dev_upload(ctx, pool, &be->plda_psi, std::vector<float>(plda_psi, plda_psi + D));
    rc |= dev_upload(ctx, pool, &be->enroll, std::vector<float>(enroll, enroll + (size_t)S * D));
    be->D = D;
    be->S = S;
    be->enroll_cap = S;
    be->threshold = threshold;
    be->logdet_given = (float)ldg;
    be->logdet_without = (float)ldw;
    return rc;
}

int plda_backend_set_enroll(sg_ctx* ctx, PldaBackend* be, std::vector<void*>& pool, const float* enroll_host, int S, float threshold) {
    if (enroll_host) {
        SG_HIP(hipSetDevice(ctx->device));
        SG_HIP(hipDeviceSynchronize());  // earlier passes may still read the table
        if (S > be->enroll_cap) {  // grow: the old table goes back to the allocator, nothing accumulates
            float* fresh = nullptr;
            int rc = dev_alloc(ctx, pool, &fresh, (size_t)S * be->D);
            if (rc) return rc;
            for (size_t i = 0; i < pool.size(); ++i)
                if (pool[i] == be->enroll) {
                    (void)hipFree(be->enroll);
                    pool.erase(pool.begin() + i);
                    break;
                }
            be->enroll = fresh;
            be->enroll_cap = S;
        }
        SG_HIP(hipMemcpy(be->enroll, enroll_host, (size_t)S * be->D * sizeof(float), hipMemcpyHostToDevice));
        be->S = S;
    }
    be->threshold = threshold;
    return SG_OK;
}

}  // namespace sg
