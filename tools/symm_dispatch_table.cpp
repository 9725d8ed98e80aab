// Prints the product kernel's host-side dispatch of a built library (host only, no device call), one line per
// (odd-DL switch, variant) and (odd-DL switch, variant, p[, K]) -- for diffing two libraries across a refactor of gemm_sym.hip:
//   g++ -std=c++17 tools/symm_dispatch_table.cpp -o /tmp/dt -Lgglasso_amd/lib -l:libggl_hip.so -Wl,-rpath,$PWD/gglasso_amd/lib
//   /tmp/dt > table.txt            (link against libggl_hip_dev.so for the development library's table)
#include <cstdio>

namespace ggl {
int symm_variants();
bool symm_variant_built(int v);
void symm_set_odd_dl(bool on);
int symm_effective_variant(int variant, int p);
int symm_auto_variant(int nprod, int p);
int symm_bounds_tile(int K, int p, int variant);
}  // namespace ggl

int main()
{
    const int ps[] = {1, 2, 15, 16, 17, 63, 64, 65, 200, 201, 500, 501, 1000};
    const int Ks[] = {1, 2, 4, 7, 8, 16, 20, 32, 64};
    printf("variants %d\n", ggl::symm_variants());
    for (int odd = 1; odd >= 0; --odd) {
        ggl::symm_set_odd_dl(odd != 0);
        for (int p : ps)
            for (int K : Ks) printf("odd_dl %d auto K %d p %d -> %d\n", odd, K, p, ggl::symm_auto_variant(K, p));
        for (int v = -1; v <= 60; ++v) {
            printf("odd_dl %d v %d built %d\n", odd, v, (int)ggl::symm_variant_built(v));
            for (int p : ps) {
                printf("odd_dl %d v %d p %d effective %d bounds", odd, v, p, ggl::symm_effective_variant(v, p));
                for (int K : Ks) printf(" %d", ggl::symm_bounds_tile(K, p, v));
                printf("\n");
            }
        }
    }
    return 0;
}
