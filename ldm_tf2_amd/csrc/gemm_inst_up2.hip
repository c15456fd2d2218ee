// gemm_kernel instantiations: MODE 4, the phase form of the upsample convolution (gemm_kernel.h), bf16_t and float
#include "gemm_launch.h"
namespace ldm_gemm_detail {
template void launch_cfg<bf16_t, 4>(int, const GemmArgs&, dim3, hipStream_t);
template void launch_cfg<float, 4>(int, const GemmArgs&, dim3, hipStream_t);
}
