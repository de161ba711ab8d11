// rt_gamma.h -- the progressive path's float -> byte conversion (realtime:1136-1147), exact by construction:
//
//     v = (double)powf(c, 1 / 2.2f);  if (!(v < 255.)) v = 255.;  (unsigned char)v
//
// with powf CORRECTLY ROUNDED -- what glibc's powf gives on every input tried, what the reference's own kernel recorded (tests/golden/ref_realtime.npz) and what exact
// arithmetic gives (tests/gamma_model.py, `decimal` at 80 digits).  The device's powf is not correctly rounded: on the 6153 values of tests/test_gpu_gamma_bytes.py it wrote
// another byte for 150 of them, all within a few floats of a code boundary.  So the byte is not computed from a power at all.  The byte does not fall as c rises, hence it
// is the NUMBER OF THRESHOLDS AT OR BELOW c: T_k (k = 1 ... 255) is the least binary32 whose byte is >= k, found by bisection over bit patterns in the exact model
// and committed below as text (tools/gen_gamma_table.py writes the lines between the markers and --check compares them; never computed from a machine's libm).
//
// Positive floats order as their bit patterns do, and the comparison is made on the bits: +0 is below T_1 (byte 0); +inf and every NaN with a clear sign bit lie
// above T_255 (byte 255, as the `!(v < 255.)` of the expression gives for inf and NaN).  A set sign bit: -0 -> powf is +0 -> 0; every negative number, -1e-45 and -inf
// included, and every NaN -> powf is NaN (+inf for -inf) -> 255.  A bounded binary search: 8 comparisons, no seed, no libm.
// Plain C++: the library's device code (accumulate_kernel) and the host library (rth_gamma_byte, tests/test_gamma_model.py) compile the same text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_GAMMA_HD __host__ __device__ __forceinline__
#else
#define RT_GAMMA_HD inline
#endif

namespace rtk {

// the byte of the correctly rounded powf(c, 1 / 2.2f) under the expression above, of the binary32 with the bits u
RT_GAMMA_HD uint32_t gamma_byte_f_bits(uint32_t u) {
    constexpr uint32_t T[255] = {
// gamma-table-begin f
    0x3f7fffffu, 0x4093088du, 0x413362a1u, 0x41a8e5a4u, 0x4209f915u, 0x424e0f40u, 0x4290a034u, 0x42c20302u,
    0x42fb6625u, 0x431e7d45u, 0x43437676u, 0x436cb347u, 0x438d2374u, 0x43a621a4u, 0x43c15ca4u, 0x43dedc6au,
    0x43fea881u, 0x4410640du, 0x4422a106u, 0x44360e74u, 0x444aaf78u, 0x44608719u, 0x4477983eu, 0x4487f2dau,
    0x4494b916u, 0x44a22024u, 0x44b02948u, 0x44bed5bbu, 0x44ce26b0u, 0x44de1d4fu, 0x44eebab8u, 0x45000002u,
    0x4508f722u, 0x45124343u, 0x451be4e7u, 0x4525dc8cu, 0x45302aafu, 0x453acfcau, 0x4545cc54u, 0x455120c2u,
    0x455ccd85u, 0x4568d30eu, 0x457531cbu, 0x4580f513u, 0x45877e46u, 0x458e34b1u, 0x45951887u, 0x459c29fau,
    0x45a3693du, 0x45aad67fu, 0x45b271efu, 0x45ba3bbeu, 0x45c23419u, 0x45ca5b2du, 0x45d2b127u, 0x45db3634u,
    0x45e3ea7fu, 0x45ecce33u, 0x45f5e17au, 0x45ff247eu, 0x46044bb4u, 0x46091d31u, 0x460e06c8u, 0x4613088fu,
    0x46182298u, 0x461d54f8u, 0x46229fc0u, 0x46280304u, 0x462d7ed7u, 0x4633134bu, 0x4638c071u, 0x463e865du,
    0x4644651fu, 0x464a5cc9u, 0x46506d6eu, 0x4656971du, 0x465cd9e7u, 0x466335dfu, 0x4669ab14u, 0x46703996u,
    0x4676e177u, 0x467da2c6u, 0x46823ecau, 0x4685b8f8u, 0x46893ff5u, 0x468cd3c8u, 0x4690747au, 0x46942211u,
    0x4697dc97u, 0x469ba411u, 0x469f7888u, 0x46a35a02u, 0x46a74888u, 0x46ab4420u, 0x46af4cd2u, 0x46b362a4u,
    0x46b7859eu, 0x46bbb5c6u, 0x46bff324u, 0x46c43dbfu, 0x46c8959cu, 0x46ccfac4u, 0x46d16d3du, 0x46d5ed0du,
    0x46da7a3au, 0x46df14cdu, 0x46e3bccau, 0x46e8723au, 0x46ed3521u, 0x46f20586u, 0x46f6e370u, 0x46fbcee4u,
    0x470063f5u, 0x4702e744u, 0x47057161u, 0x47080250u, 0x470a9a14u, 0x470d38b0u, 0x470fde26u, 0x47128a7au,
    0x47153dafu, 0x4717f7c7u, 0x471ab8c6u, 0x471d80aeu, 0x47204f83u, 0x47232547u, 0x472601fcu, 0x4728e5a7u,
    0x472bd048u, 0x472ec1e4u, 0x4731ba7du, 0x4734ba17u, 0x4737c0b2u, 0x473ace53u, 0x473de2fcu, 0x4740feb0u,
    0x47442171u, 0x47474b42u, 0x474a7c25u, 0x474db41eu, 0x4750f32eu, 0x47543959u, 0x475786a1u, 0x475adb08u,
    0x475e3692u, 0x47619940u, 0x47650315u, 0x47687413u, 0x476bec3eu, 0x476f6b98u, 0x4772f222u, 0x47767fe0u,
    0x477a14d4u, 0x477db100u, 0x4780aa34u, 0x47827f86u, 0x47845878u, 0x4786350au, 0x4788153fu, 0x4789f917u,
    0x478be094u, 0x478dcbb6u, 0x478fba80u, 0x4791acf1u, 0x4793a30bu, 0x47959ccfu, 0x47979a3fu, 0x47999b5bu,
    0x479ba025u, 0x479da89eu, 0x479fb4c6u, 0x47a1c4a0u, 0x47a3d82bu, 0x47a5ef6au, 0x47a80a5du, 0x47aa2905u,
    0x47ac4b63u, 0x47ae717au, 0x47b09b48u, 0x47b2c8d1u, 0x47b4fa14u, 0x47b72f13u, 0x47b967ceu, 0x47bba448u,
    0x47bde480u, 0x47c02879u, 0x47c27032u, 0x47c4bbadu, 0x47c70aecu, 0x47c95deeu, 0x47cbb4b6u, 0x47ce0f43u,
    0x47d06d98u, 0x47d2cfb5u, 0x47d5359bu, 0x47d79f4bu, 0x47da0cc6u, 0x47dc7e0eu, 0x47def322u, 0x47e16c04u,
    0x47e3e8b6u, 0x47e66937u, 0x47e8ed8au, 0x47eb75aeu, 0x47ee01a6u, 0x47f09171u, 0x47f32511u, 0x47f5bc86u,
    0x47f857d3u, 0x47faf6f7u, 0x47fd99f4u, 0x48002065u, 0x480175beu, 0x4802cd04u, 0x48042638u, 0x4805815bu,
    0x4806de6du, 0x48083d6eu, 0x48099e5fu, 0x480b0141u, 0x480c6614u, 0x480dccd8u, 0x480f358eu, 0x4810a036u,
    0x48120cd1u, 0x48137b5fu, 0x4814ebe1u, 0x48165e56u, 0x4817d2c0u, 0x4819491fu, 0x481ac174u, 0x481c3bbeu,
    0x481db7feu, 0x481f3635u, 0x4820b663u, 0x48223888u, 0x4823bca6u, 0x482542bcu, 0x4826cacau, 0x482854d2u,
    0x4829e0d3u, 0x482b6ecfu, 0x482cfec5u, 0x482e90b5u, 0x483024a1u, 0x4831ba89u, 0x4833526du, 0x4834ec4du,
    0x4836882bu, 0x48382606u, 0x4839c5deu, 0x483b67b5u, 0x483d0b8au, 0x483eb15eu, 0x48405932u
// gamma-table-end
    };
    if (u & 0x80000000u) return u == 0x80000000u ? 0u : 255u;
    uint32_t n = 0;                                               // the number of k with T_k <= u: T[n - 1] <= u < T[n]
    for (uint32_t step = 128; step != 0; step >>= 1)
        if (n + step <= 255u && T[n + step - 1] <= u) n += step;
    return n;
}

RT_GAMMA_HD uint32_t gamma_byte_f(float c) {
    uint32_t u;
    __builtin_memcpy(&u, &c, 4);
    return gamma_byte_f_bits(u);
}

}  // namespace rtk
