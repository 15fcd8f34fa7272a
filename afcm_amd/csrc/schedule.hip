// The three scalars of the reference's training loop that change over time -- the loss-side blur sigma (models/stylegan3_model.py:115-116), the EMA
// beta (train.py:67-73) and the learning rates (models/utils.py:43-69) -- in one DEVICE block of 8 doubles, so that a captured graph reads them at
// every replay instead of carrying the launch scalars of the step it was captured from.
//   schedule_advance_kernel   one thread: total_iters += batch, then sigma, radius and beta from it; the learning-rate slots are the host's
// sigma and radius use + - x / floor max in double only, and the library is built with -ffp-contract=off: they are bit-equal to the Python expressions.
#include "common.h"

namespace afcm {

__global__ void schedule_advance_kernel(double* __restrict__ block, long long batch, double blur_init_sigma, double blur_fade_kimg, double ema_kimgs,
                                        double ema_ramp) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double total = block[0] + (double)batch;
    double sigma = 0.0;
    if (blur_fade_kimg > 0.0) {
        const double left = 1.0 - total / (blur_fade_kimg * 1e3);              // max(1 - cur_nimg / (blur_fade_kimg * 1e3), 0) * blur_init_sigma
        sigma = (left > 0.0 ? left : 0.0) * blur_init_sigma;
    }
    double ema_nimg = ema_kimgs * 1000.0;
    if (ema_ramp >= 0.0) {
        const double ramped = total * ema_ramp;
        ema_nimg = ramped < ema_nimg ? ramped : ema_nimg;                      // min(ema_nimg, total_iters * ramp)
    }
    block[0] = total;
    block[1] = sigma;
    block[2] = floor(sigma * 3.0);
    block[3] = pow(0.5, (double)batch / (ema_nimg > 1e-8 ? ema_nimg : 1e-8));
}

}  // namespace afcm

extern "C" int afcm_schedule_advance(double* block, int64_t batch, double blur_init_sigma, double blur_fade_kimg, double ema_kimgs, double ema_ramp,
                                     void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(block != nullptr, "schedule_advance: null block");
    AFCM_REQUIRE(batch >= 1, "schedule_advance: batch %lld is below 1", (long long)batch);
    hipLaunchKernelGGL(schedule_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, block, (long long)batch, blur_init_sigma, blur_fade_kimg,
                       ema_kimgs, ema_ramp);
    return hip_status(hipGetLastError());
}
