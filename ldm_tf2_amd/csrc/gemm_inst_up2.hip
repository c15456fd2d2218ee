// gemm_kernel instantiations: MODE 4, the phase form of the upsample convolution (gemm_kernel.h), bf16_t and float
#include "gemm_launch.h"
namespace ldm_gemm_detail {
template void launch_phase<bf16_t>(int, const GemmArgs&, dim3, hipStream_t);
template void launch_phase<float>(int, const GemmArgs&, dim3, hipStream_t);
}
