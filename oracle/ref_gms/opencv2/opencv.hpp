// Stand-in for <opencv2/opencv.hpp>: only the names the reference's src/utils/GMSMatcher/gms_matcher.{h,cpp} use, so that those
// two files compile unchanged with a plain C++ compiler (`make ref`, oracle/ref_gms/gms_ref.cc).  Test infrastructure only.
//
//   * <cmath> is included here, as OpenCV's core headers do: gms_matcher.h calls floor() unqualified under `using namespace std`, and
//     which overload that picks (std::floor(float) for a float argument) depends on <cmath> being visible.
//   * Mat stores int (the reference only creates CV_32SC1 matrices) and CHECKS every row / element access.  An access outside the
//     matrix sets ref_gms::out_of_bounds and leaves by an exception (caught in gms_ref.cc): the reference follows its matrix access by
//     a std::vector access with the same index (gms_matcher.cpp:94-95), which a stand-in cannot redirect, so an undefined input is
//     detected at the first access and never executed.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#define CV_32SC1 4

namespace ref_gms {
extern int out_of_bounds;
struct OutOfBounds {};
[[noreturn]] inline void fail() { out_of_bounds = 1; throw OutOfBounds(); }
}  // namespace ref_gms

namespace cv {

struct Point2f {
    float x, y;
    Point2f() : x(0.f), y(0.f) {}
    Point2f(float x_, float y_) : x(x_), y(y_) {}
};

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct KeyPoint {
    Point2f pt;
};

struct DMatch {
    int queryIdx, trainIdx;
    DMatch() : queryIdx(-1), trainIdx(-1) {}
    DMatch(int q, int t) : queryIdx(q), trainIdx(t) {}
};

struct Scalar {
    double val[4];
    double operator[](int i) const { return val[i]; }
};

class Mat {
public:
    int rows, cols;
    Mat() : rows(0), cols(0) {}
    static Mat zeros(int r, int c, int /*type*/)
    {
        Mat m;
        m.rows = r; m.cols = c;
        m.data_.assign((size_t)r * (size_t)c, 0);
        return m;
    }
    template <typename T> T *ptr(int r)
    {
        static_assert(sizeof(T) == sizeof(int), "the stand-in Mat holds int");
        if (r < 0 || r >= rows) ref_gms::fail();
        return data_.data() + (size_t)r * (size_t)cols;
    }
    template <typename T> const T *ptr(int r) const { return const_cast<Mat *>(this)->ptr<T>(r); }
    template <typename T> T &at(int r, int c)
    {
        if (c < 0 || c >= cols) ref_gms::fail();
        return ptr<T>(r)[c];
    }
    void setTo(int v) { data_.assign(data_.size(), v); }
    Mat row(int r) const
    {
        const int *p = ptr<int>(r);
        Mat m = zeros(1, cols, CV_32SC1);
        if (cols > 0) std::memcpy(m.data_.data(), p, sizeof(int) * (size_t)cols);
        return m;
    }
    const std::vector<int> &elements() const { return data_; }

private:
    std::vector<int> data_;
};

inline Scalar sum(const Mat &m)
{
    Scalar s = {{0, 0, 0, 0}};
    for (int v : m.elements()) s.val[0] += v;
    return s;
}
inline Scalar sum(const std::vector<bool> &b)
{
    Scalar s = {{0, 0, 0, 0}};
    for (bool v : b) s.val[0] += v ? 1 : 0;
    return s;
}

}  // namespace cv
