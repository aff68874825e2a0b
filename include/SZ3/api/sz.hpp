// SZ3/api/sz.hpp — source-compatible C++ face of libsz3hip.so (MI355X-native SZ3 hot path).
//
// A program written against the reference's public header (`#include "SZ3/api/sz.hpp"`, e.g. the reference CLI
// tools/sz3/sz3.cpp or the HDF5 filter tools/H5Z-SZ3/src/H5Z_SZ3.cpp) compiles unchanged with `-I<this repo>/include`
// and links `-lsz3hip`; the four entry points below then run on the GPU through the C ABI of include/sz3hip.h.
// This file holds NO compression code: every template forwards to sz3hip_compress / sz3hip_decompress.
//
// Interfaces replaced (reference file:line):
//   SZ_compress<T>(conf, data, cmpData, cmpCap) -> size      include/SZ3/api/sz.hpp:43
//   SZ_compress<T>(conf, data, cmpSize&) -> new char[]       include/SZ3/api/sz.hpp:94
//   SZ_decompress<T>(conf, cmpData, cmpSize, T*& decData)    include/SZ3/api/sz.hpp:117
//   SZ_decompress<T>(conf, cmpData, cmpSize) -> new T[]      include/SZ3/api/sz.hpp:172
//   SZ_compress_size_bound<T>(conf)                          include/SZ3/api/impl/SZImpl.hpp:34
//   SZ3::Config (fields, ctor, setDims, loadcfg/load_ini/save_ini, save/load, print)   include/SZ3/utils/Config.hpp:142-478
//   SZ3::EB / ALGO / INTERP_ALGO enums and *_MAP tables, match_enum, enum_to_string     include/SZ3/utils/Config.hpp:47-133
//   SZ3::readfile / writefile / writeTextFile                include/SZ3/utils/FileUtil.hpp:25-80
//   SZ3::verify                                              include/SZ3/utils/Statistic.hpp:79-160
//   SZ3::Timer                                               include/SZ3/utils/Timer.hpp
// Error behaviour as in the reference: std::invalid_argument / std::length_error / std::runtime_error carrying
// sz3hip_last_error() (api/sz.hpp:47-49, 122-135).
#ifndef SZ3HIP_CXX_SZ_HPP
#define SZ3HIP_CXX_SZ_HPP

#include <algorithm>
#include <cassert>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../sz3hip.h"

#define SZ3_VER "3.3.2"
#define SZ3_VER_MAJOR 3
#define SZ3_VER_MINOR 3
#define SZ3_VER_PATCH 2
#define SZ3_VER_TWEAK 0
#define SZ3_DATA_VER "3.3.2"
#define SZ3_MAGIC_NUMBER 0xF342F310u

#define SZ_FLOAT 0
#define SZ_DOUBLE 1
#define SZ_UINT8 2
#define SZ_INT8 3
#define SZ_UINT16 4
#define SZ_INT16 5
#define SZ_UINT32 6
#define SZ_INT32 7
#define SZ_UINT64 8
#define SZ_INT64 9

namespace SZ3 {

typedef unsigned int uint;
typedef unsigned char uchar;

enum EB { EB_ABS, EB_REL, EB_PSNR, EB_L2NORM, EB_ABS_AND_REL, EB_ABS_OR_REL };
enum ALGO { ALGO_LORENZO_REG, ALGO_INTERP_LORENZO, ALGO_INTERP, ALGO_NOPRED, ALGO_LOSSLESS, ALGO_BIOMD, ALGO_BIOMDXTC,
            ALGO_HIP_LORENZO = SZ3HIP_ALGO_HIP_LORENZO, ALGO_HIP_INTERP = SZ3HIP_ALGO_HIP_INTERP };
enum INTERP_ALGO { INTERP_ALGO_LINEAR, INTERP_ALGO_CUBIC };

static const std::map<std::string, ALGO> ALGO_MAP = {
    {"ALGO_LORENZO_REG", ALGO_LORENZO_REG}, {"ALGO_INTERP_LORENZO", ALGO_INTERP_LORENZO}, {"ALGO_INTERP", ALGO_INTERP},
    {"ALGO_NOPRED", ALGO_NOPRED},           {"ALGO_LOSSLESS", ALGO_LOSSLESS},             {"ALGO_BIOMD", ALGO_BIOMD},
    {"ALGO_BIOMDXTC", ALGO_BIOMDXTC},       {"ALGO_HIP_LORENZO", ALGO_HIP_LORENZO},       {"ALGO_HIP_INTERP", ALGO_HIP_INTERP}};
static const std::map<std::string, EB> EB_MAP = {{"ABS", EB_ABS},       {"REL", EB_REL},
                                                 {"PSNR", EB_PSNR},     {"NORM", EB_L2NORM},
                                                 {"ABS_AND_REL", EB_ABS_AND_REL}, {"ABS_OR_REL", EB_ABS_OR_REL}};
static const std::map<std::string, INTERP_ALGO> INTERP_ALGO_MAP = {{"INTERP_ALGO_LINEAR", INTERP_ALGO_LINEAR},
                                                                   {"INTERP_ALGO_CUBIC", INTERP_ALGO_CUBIC}};

inline std::string to_lower(std::string s) {
    for (auto &ch : s) ch = (char)std::tolower((unsigned char)ch);
    return s;
}
// case-insensitive lookup of a table key; `out` is left alone when nothing matches (Config.hpp:105-113)
template <typename E>
inline void match_enum(const std::string &text, const std::map<std::string, E> &table, uint8_t &out) {
    const std::string want = to_lower(text);
    for (const auto &kv : table)
        if (to_lower(kv.first) == want) out = (uint8_t)kv.second;
}
template <typename E>
inline std::string enum_to_string(E value, const std::map<std::string, E> &table) {
    for (const auto &kv : table)
        if (kv.second == value) return kv.first;
    return std::string();
}
inline uint32_t versionInt(const std::string &v) {  // "3.3.2" -> 0x03030200 (version.hpp.in)
    unsigned a = 0, b = 0, c = 0, d = 0;
    std::sscanf(v.c_str(), "%u.%u.%u.%u", &a, &b, &c, &d);
    return (a << 24) | (b << 16) | (c << 8) | d;
}
inline std::string versionStr(uint32_t v) {
    std::ostringstream s;
    s << (v >> 24) << '.' << ((v >> 16) & 0xFF) << '.' << ((v >> 8) & 0xFF) << '.' << (v & 0xFF);
    return s.str();
}

class Config {
   public:
    template <class... Dims>
    Config(Dims... args) {
        std::vector<size_t> d{static_cast<size_t>(args)...};
        setDims(d.begin(), d.end());
    }
    Config(std::initializer_list<size_t> d) { setDims(d.begin(), d.end()); }

    template <class Iter>
    size_t setDims(Iter begin, Iter end) {
        uint64_t raw[16];
        int nd = 0;
        for (Iter it = begin; it != end && nd < 16; ++it) raw[nd++] = (uint64_t)*it;
        // the library applies the reference's rules (size-1 dims dropped, predDim, blockSize per N); only the
        // geometry is taken from the result so that user-set fields survive a later setDims (Config.hpp:160-177)
        uint64_t kept[4];
        int nk = 0;
        for (int i = 0; i < nd; i++)
            if (raw[i] > 1) {
                if (nk == 4) throw std::invalid_argument("SZ3 (HIP): more than 4 dimensions above size 1");
                kept[nk++] = raw[i];
            }
        if (nk == 0) kept[nk++] = 1;
        sz3hip_config pod;
        sz3hip_config_init(&pod, nk, kept);
        dims.assign(kept, kept + nk);
        N = (char)pod.N;
        num = (size_t)pod.num;
        predDim = pod.predDim;
        blockSize = pod.blockSize;
        return num;
    }

    void loadcfg(const std::string &path) {
        std::ifstream f(path);
        if (!f.is_open()) throw std::runtime_error("Failed to open INI file: " + path);
        std::ostringstream all;
        all << f.rdbuf();
        load_ini(all.str());
    }

    // INI dialect of the reference (Config.hpp:196-266): [GlobalSettings] / [AlgoSettings], `key = value`,
    // '#' comments, keys and enum names case-insensitive. Table-driven here.
    void load_ini(const std::string &text) {
        auto strip = [](std::string s) {
            const char *ws = " \t\r\n";
            const size_t a = s.find_first_not_of(ws);
            if (a == std::string::npos) return std::string();
            return s.substr(a, s.find_last_not_of(ws) - a + 1);
        };
        auto truth = [](const std::string &v) {
            const std::string l = to_lower(v);
            return l == "true" || l == "1" || l == "yes" || l == "on";
        };
        typedef std::function<void(const std::string &)> Setter;
        const std::map<std::string, Setter> keys = {
            {"globalsettings/cmpralgo", [&](const std::string &v) { match_enum(v, ALGO_MAP, cmprAlgo); }},
            {"globalsettings/errorboundmode", [&](const std::string &v) { match_enum(v, EB_MAP, errorBoundMode); }},
            {"globalsettings/abserrorbound", [&](const std::string &v) { absErrorBound = std::stod(v); }},
            {"globalsettings/relerrorbound", [&](const std::string &v) { relErrorBound = std::stod(v); }},
            {"globalsettings/psnrerrorbound", [&](const std::string &v) { psnrErrorBound = std::stod(v); }},
            {"globalsettings/l2normerrorbound", [&](const std::string &v) { l2normErrorBound = std::stod(v); }},
            {"globalsettings/openmp", [&](const std::string &v) { openmp = truth(v); }},
            {"algosettings/lorenzo", [&](const std::string &v) { lorenzo = truth(v); }},
            {"algosettings/lorenzo2ndorder", [&](const std::string &v) { lorenzo2 = truth(v); }},
            {"algosettings/regression", [&](const std::string &v) { regression = truth(v); }},
            {"algosettings/regression2ndorder", [&](const std::string &v) { regression2 = truth(v); }},
            {"algosettings/interpolationalgo", [&](const std::string &v) { match_enum(v, INTERP_ALGO_MAP, interpAlgo); }},
            {"algosettings/interpolationdirection", [&](const std::string &v) { interpDirection = (uint8_t)std::stoi(v); }},
            {"algosettings/blocksize", [&](const std::string &v) { blockSize = std::stoi(v); }},
            {"algosettings/quantizationbintotal", [&](const std::string &v) { quantbinCnt = std::stoi(v); }},
            {"algosettings/interpolationanchorstride", [&](const std::string &v) { interpAnchorStride = std::stoi(v); }},
            {"algosettings/interpolationalpha", [&](const std::string &v) { interpAlpha = std::stod(v); }},
            {"algosettings/interpolationbeta", [&](const std::string &v) { interpBeta = std::stod(v); }},
        };
        std::istringstream in(text);
        std::string line, section;
        while (std::getline(in, line)) {
            line = strip(line);
            if (line.empty() || line[0] == '#') continue;
            if (line[0] == '[') {
                section = to_lower(line.substr(1, line.find(']') - 1));
                continue;
            }
            const size_t eq = line.find('=');
            if (eq == std::string::npos) continue;
            auto hit = keys.find(section + "/" + to_lower(strip(line.substr(0, eq))));
            if (hit != keys.end()) hit->second(strip(line.substr(eq + 1)));
        }
    }

    std::string save_ini() const {
        std::ostringstream o;
        auto b = [](bool v) { return v ? "true" : "false"; };
        o << "[GlobalSettings]\n"
          << "CmprAlgo = " << enum_to_string((ALGO)cmprAlgo, ALGO_MAP) << "\n"
          << "ErrorBoundMode = " << enum_to_string((EB)errorBoundMode, EB_MAP) << "\n"
          << "AbsErrorBound = " << absErrorBound << "\n"
          << "RelErrorBound = " << relErrorBound << "\n"
          << "PSNRErrorBound = " << psnrErrorBound << "\n"
          << "L2NormErrorBound = " << l2normErrorBound << "\n"
          << "OpenMP = " << b(openmp) << "\n\n[AlgoSettings]\n"
          << "Lorenzo = " << b(lorenzo) << "\n"
          << "Lorenzo2ndOrder = " << b(lorenzo2) << "\n"
          << "Regression = " << b(regression) << "\n"
          << "Regression2ndOrder = " << b(regression2) << "\n"
          << "BlockSize = " << blockSize << "\n"
          << "QuantizationBinTotal = " << quantbinCnt << "\n"
          << "InterpolationAlgo = " << enum_to_string((INTERP_ALGO)interpAlgo, INTERP_ALGO_MAP) << "\n"
          << "InterpolationDirection = " << (int)interpDirection << "\n"
          << "InterpolationAnchorStride = " << interpAnchorStride << "\n"
          << "InterpolationAlpha = " << interpAlpha << "\n"
          << "InterpolationBeta = " << interpBeta << "\n";
        return o.str();
    }

    // byte layout of Config::save/load (Config.hpp:312-413) — produced and parsed by the library
    size_t save(unsigned char *&c) const {
        const sz3hip_config pod = to_pod();
        const size_t n = sz3hip_config_save(&pod, c);
        c += n;
        return n;
    }
    void load(const unsigned char *&c) {
        sz3hip_config pod;
        const size_t n = sz3hip_config_load(&pod, c);
        if (n == 0) throw std::invalid_argument(sz3hip_last_error());
        from_pod(pod);
        c += n;
    }
    size_t size_est() const {
        std::vector<unsigned char> tmp(512);
        unsigned char *p = tmp.data();
        return save(p);
    }
    void print() const { std::cout << save_ini() << std::endl; }

    sz3hip_config to_pod() const {
        sz3hip_config p;
        std::memset(&p, 0, sizeof(p));
        p.N = N;
        for (size_t i = 0; i < dims.size() && i < 4; i++) p.dims[i] = dims[i];
        p.num = num;
        p.cmprAlgo = cmprAlgo;
        p.errorBoundMode = errorBoundMode;
        p.absErrorBound = absErrorBound;
        p.relErrorBound = relErrorBound;
        p.psnrErrorBound = psnrErrorBound;
        p.l2normErrorBound = l2normErrorBound;
        p.openmp = openmp;
        p.quantbinCnt = quantbinCnt;
        p.blockSize = blockSize;
        p.predDim = predDim;
        p.dataType = dataType;
        p.lorenzo = lorenzo;
        p.lorenzo2 = lorenzo2;
        p.regression = regression;
        p.regression2 = regression2;
        p.interpAlgo = interpAlgo;
        p.interpDirection = interpDirection;
        p.interpAnchorStride = interpAnchorStride;
        p.interpAlpha = interpAlpha;
        p.interpBeta = interpBeta;
        return p;
    }
    void from_pod(const sz3hip_config &p) {
        N = (char)p.N;
        dims.assign(p.dims, p.dims + p.N);
        num = (size_t)p.num;
        cmprAlgo = p.cmprAlgo;
        errorBoundMode = p.errorBoundMode;
        absErrorBound = p.absErrorBound;
        relErrorBound = p.relErrorBound;
        psnrErrorBound = p.psnrErrorBound;
        l2normErrorBound = p.l2normErrorBound;
        openmp = p.openmp != 0;
        quantbinCnt = p.quantbinCnt;
        blockSize = p.blockSize;
        predDim = p.predDim;
        dataType = p.dataType;
        lorenzo = p.lorenzo != 0;
        lorenzo2 = p.lorenzo2 != 0;
        regression = p.regression != 0;
        regression2 = p.regression2 != 0;
        interpAlgo = p.interpAlgo;
        interpDirection = p.interpDirection;
        interpAnchorStride = p.interpAnchorStride;
        interpAlpha = p.interpAlpha;
        interpBeta = p.interpBeta;
    }

    uint32_t sz3MagicNumber = SZ3_MAGIC_NUMBER;
    uint32_t sz3DataVer = versionInt(SZ3_DATA_VER);
    char N = 0;
    std::vector<size_t> dims;
    size_t num = 0;
    uint8_t cmprAlgo = ALGO_INTERP_LORENZO;
    uint8_t errorBoundMode = EB_ABS;
    double absErrorBound = 1e-3;
    double relErrorBound = 0.0;
    double psnrErrorBound = 0.0;
    double l2normErrorBound = 0.0;
    bool openmp = false;
    int quantbinCnt = 65536;
    int blockSize = 0;
    uint8_t predDim = 0;
    uint8_t dataType = SZ_FLOAT;
    bool lorenzo = true;
    bool lorenzo2 = false;
    bool regression = true;
    bool regression2 = false;
    uint8_t interpAlgo = INTERP_ALGO_CUBIC;
    uint8_t interpDirection = 0;
    int interpAnchorStride = -1;
    double interpAlpha = 1.25;
    double interpBeta = 2.0;
};

// ---- small utilities the reference's tools use --------------------------------------------------------------
class Timer {
   public:
    Timer() = default;
    explicit Timer(bool go) {
        if (go) start();
    }
    void start() { t0_ = clock_t_::now(); }
    double stop() { return std::chrono::duration<double>(clock_t_::now() - t0_).count(); }
    double stop(const std::string &msg) {
        const double s = stop();
        std::cout << msg << " time = " << s << "s" << std::endl;
        return s;
    }

   private:
    typedef std::chrono::steady_clock clock_t_;
    clock_t_::time_point t0_;
};

template <typename Type>
void readfile(const char *file, const size_t num, Type *data) {
    std::ifstream f(file, std::ios::binary);
    if (!f) throw std::invalid_argument(std::string("Error, Couldn't find the file: ") + file);
    f.seekg(0, std::ios::end);
    const size_t have = (size_t)f.tellg() / sizeof(Type);
    if (have != num) throw std::invalid_argument("The input file size does not match the given dimensions");
    f.seekg(0, std::ios::beg);
    f.read(reinterpret_cast<char *>(data), (std::streamsize)(num * sizeof(Type)));
}
template <typename Type>
std::unique_ptr<Type[]> readfile(const char *file, size_t &num) {
    std::ifstream f(file, std::ios::binary);
    if (!f) throw std::invalid_argument(std::string("Error, Couldn't find the file: ") + file);
    f.seekg(0, std::ios::end);
    num = (size_t)f.tellg() / sizeof(Type);
    f.seekg(0, std::ios::beg);
    std::unique_ptr<Type[]> data(new Type[num]);
    f.read(reinterpret_cast<char *>(data.get()), (std::streamsize)(num * sizeof(Type)));
    return data;
}
template <typename Type>
void writefile(const char *file, Type *data, size_t num_elements) {
    std::ofstream f(file, std::ios::binary);
    f.write(reinterpret_cast<const char *>(data), (std::streamsize)(num_elements * sizeof(Type)));
}
template <typename Type>
void writeTextFile(const char *file, Type *data, size_t num_elements) {
    std::ofstream f(file);
    if (!f) throw std::invalid_argument(std::string("Error, Couldn't open the file: ") + file);
    for (size_t i = 0; i < num_elements; i++) f << data[i] << std::endl;
}

// error statistics of a round trip (Statistic.hpp:79-160): PSNR over the value range, NRMSE, max abs diff
template <typename Type>
void verify(Type *ori, Type *dec, size_t n, double &psnr, double &nrmse, double &max_diff) {
    double lo = (double)ori[0], hi = lo, sq = 0, mx = 0, so = 0, sd = 0;
    for (size_t i = 0; i < n; i++) {
        const double a = (double)ori[i], b = (double)dec[i], e = std::fabs(a - b);
        lo = std::min(lo, a);
        hi = std::max(hi, a);
        mx = std::max(mx, e);
        sq += e * e;
        so += a;
        sd += b;
    }
    const double mo = so / n, md = sd / n, range = hi - lo, mse = sq / n;
    double cov = 0, vo = 0, vd = 0, max_rel = 0;
    for (size_t i = 0; i < n; i++) {
        const double a = (double)ori[i] - mo, b = (double)dec[i] - md;
        cov += a * b;
        vo += a * a;
        vd += b * b;
        if (ori[i] != 0) max_rel = std::max(max_rel, std::fabs(((double)ori[i] - (double)dec[i]) / (double)ori[i]));
    }
    psnr = 20 * std::log10(range) - 10 * std::log10(mse);
    nrmse = std::sqrt(mse) / range;
    max_diff = mx;
    std::printf("Min=%.20G, Max=%.20G, range=%.20G\n", lo, hi, range);
    std::printf("Max absolute error = %.2G\n", mx);
    std::printf("Max relative error = %.2G\n", range > 0 ? mx / range : 0.0);
    std::printf("Max pw relative error = %.2G\n", max_rel);
    std::printf("PSNR = %f, NRMSE= %.10G\n", psnr, nrmse);
    std::printf("L2 error = %.10G\n", std::sqrt(sq));
    std::printf("acEff=%f\n", (vo > 0 && vd > 0) ? cov / std::sqrt(vo * vd) : 1.0);
}
template <typename Type>
void verify(Type *ori, Type *dec, size_t n) {
    double a, b, c;
    verify(ori, dec, n, a, b, c);
}
template <typename Type>
void verify(Type *ori, Type *dec, size_t n, double &psnr, double &nrmse) {
    double c;
    verify(ori, dec, n, psnr, nrmse, c);
}

// (libsz3hip) streams stock SZ3 reads: SZ_compress writes cmprAlgo ALGO_INTERP in the reference's own container wherever the interpolation
// predictor is chosen — the default ALGO_INTERP_LORENZO's outcome on most data; reading stock ALGO_INTERP streams needs no switch
inline void hip_stock_format(bool on) { sz3hip_set_stock_format(on ? 1 : 0); }

namespace hipdetail {
template <class T>
inline int dtype_of() {
    if (std::is_same<T, float>::value) return SZ3HIP_FLOAT;
    if (std::is_same<T, double>::value) return SZ3HIP_DOUBLE;
    if (std::is_integral<T>::value && !std::is_same<T, bool>::value) {  // (the ten types of tools/H5Z-SZ3/src/H5Z_SZ3.cpp:195-227)
        const bool sg = std::is_signed<T>::value;
        switch (sizeof(T)) {
            case 1: return sg ? SZ3HIP_INT8 : SZ3HIP_UINT8;
            case 2: return sg ? SZ3HIP_INT16 : SZ3HIP_UINT16;
            case 4: return sg ? SZ3HIP_INT32 : SZ3HIP_UINT32;
            case 8: return sg ? SZ3HIP_INT64 : SZ3HIP_UINT64;
        }
    }
    throw std::invalid_argument("SZ3 (HIP path): float, double and 8 / 16 / 32 / 64-bit integer arrays are supported by libsz3hip");
}
[[noreturn]] inline void raise_last(int code) {
    const std::string msg = sz3hip_last_error();
    if (code == SZ3HIP_ECAPACITY) throw std::length_error(msg);
    if (code == SZ3HIP_EINVAL || code == SZ3HIP_EFORMAT) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}
}  // namespace hipdetail

// (libsz3hip) the numbers of verify() above for two contiguous arrays of n elements in DEVICE memory, reduced on the device that holds
// them (sz3hip_verify_device: each array read once, nothing printed); bound >= 0: n_over / first_over count |dec - ori| > bound.
// stream: what is waited for before the arrays are read. Errors are the exceptions of the entry points below.
template <class T>
inline sz3hip_verify_stats hip_verify_device(const T *d_ori, const T *d_dec, size_t n, double bound = -1, void *stream = nullptr) {
    const uint64_t dims[1] = {(uint64_t)n};
    sz3hip_verify_stats st;
    const int rc = sz3hip_verify_device(hipdetail::dtype_of<T>(), 1, dims, d_ori, nullptr, d_dec, nullptr, bound, &st, stream);
    if (rc) hipdetail::raise_last(rc);
    return st;
}

}  // namespace SZ3

// ---- the four entry points (global namespace, as in the reference) --------------------------------------------
template <class T>
size_t SZ_compress_size_bound(const SZ3::Config &conf) {
    const sz3hip_config pod = conf.to_pod();
    return sz3hip_compress_bound(&pod, SZ3::hipdetail::dtype_of<T>());
}

template <class T>
size_t SZ_compress(const SZ3::Config &config, const T *data, char *cmpData, size_t cmpCap) {
    const sz3hip_config pod = config.to_pod();
    const int dt = SZ3::hipdetail::dtype_of<T>();
    const size_t n = sz3hip_compress(&pod, dt, data, cmpData, cmpCap);
    if (n == 0) SZ3::hipdetail::raise_last(sz3hip_last_error_code());
    return n;
}

template <class T>
char *SZ_compress(const SZ3::Config &config, const T *data, size_t &cmpSize) {
    const size_t cap = SZ_compress_size_bound<T>(config);
    std::unique_ptr<char[]> buf(new char[cap]);
    cmpSize = SZ_compress<T>(config, data, buf.get(), cap);
    return buf.release();
}

template <class T>
void SZ_decompress(SZ3::Config &config, const char *cmpData, size_t cmpSize, T *&decData) {
    sz3hip_config pod;
    int rc = sz3hip_peek_config(&pod, cmpData, cmpSize);
    if (rc != 0) SZ3::hipdetail::raise_last(rc);
    const bool own = decData == nullptr;
    if (own) decData = new T[pod.num];
    rc = sz3hip_decompress(&pod, SZ3::hipdetail::dtype_of<T>(), cmpData, cmpSize, decData);
    if (rc != 0) {
        if (own) {
            delete[] decData;
            decData = nullptr;
        }
        SZ3::hipdetail::raise_last(rc);
    }
    config.from_pod(pod);
}

template <class T>
T *SZ_decompress(SZ3::Config &config, const char *cmpData, size_t cmpSize) {
    T *out = nullptr;
    SZ_decompress<T>(config, cmpData, cmpSize, out);
    return out;
}

#endif  // SZ3HIP_CXX_SZ_HPP
