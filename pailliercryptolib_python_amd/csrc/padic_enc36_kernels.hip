// 36-limb instantiations of the base-n digit-pair kernels: n of 700..1024 bits (1024-bit keys), 12-row blocks.
#include "padic_enc_launch.hpp"

namespace pai {

using L36 = EncLaunch<36, 12>;
const PadicEncOps* padic_enc_ops_36() {
    static const PadicEncOps o = enc_ops<L36, L36>();
    return &o;
}

}  // namespace pai
