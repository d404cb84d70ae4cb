// A stand-in for the part of OpenCV that the reference's Tool/IO.cpp, Tool/ImageProcessing.cpp, Geometry/*.cpp and Integration/*.cpp touch, so that those
// units compile and link in a container without OpenCV (tests/tools/gen_align_color_golden.py, oracle/tools/gen_volume_golden.py).  A continuous row-major image container and the names
// the headers mention; the image-processing calls are declared here and defined as aborting stubs in main.cpp -- the generator never reaches them.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <iomanip>
#include <iostream>
#include <map>
#include <unordered_map>
#include <string>
#include <cstring>
#include <memory>
#include <vector>

#define CV_8U 0
#define CV_16U 2
#define CV_32F 5
#define CV_MAKETYPE(depth, cn) (((depth) & 7) + (((cn) - 1) << 3))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_16UC1 CV_MAKETYPE(CV_16U, 1)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_RGB2GRAY 7

namespace cv {
struct Vec3b {
    unsigned char val[3];
    unsigned char& operator[](int i) { return val[i]; }
    const unsigned char& operator[](int i) const { return val[i]; }
};
struct Scalar {
    double v[4];
    Scalar(double a = 0, double b = 0, double c = 0, double d = 0) { v[0] = a; v[1] = b; v[2] = c; v[3] = d; }
};
struct Size { int width, height; Size(int w = 0, int h = 0) : width(w), height(h) {} };
struct KeyPoint {};
struct DMatch {};

class Mat {
  public:
    int rows = 0, cols = 0;
    unsigned char* data = nullptr;
    Mat() = default;
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(int r, int c, int type, const Scalar& s) {
        create(r, c, type);
        const int cn = channels();
        for (size_t i = 0; i < (size_t)r * c; ++i)
            for (int k = 0; k < cn; ++k) {
                if (depth() == CV_8U) data[i * cn + k] = (unsigned char)s.v[k];
                else if (depth() == CV_16U) reinterpret_cast<unsigned short*>(data)[i * cn + k] = (unsigned short)s.v[k];
                else reinterpret_cast<float*>(data)[i * cn + k] = (float)s.v[k];
            }
    }
    void create(int r, int c, int type) {
        rows = r; cols = c; type_ = type;
        buf_ = std::make_shared<std::vector<unsigned char> >((size_t)r * c * elemSize());
        data = buf_->empty() ? nullptr : buf_->data();
    }
    void release() { rows = cols = 0; data = nullptr; buf_.reset(); }
    int type() const { return type_; }
    int depth() const { return type_ & 7; }
    int channels() const { return (type_ >> 3) + 1; }
    size_t elemSize() const { return (depth() == CV_8U ? 1 : depth() == CV_16U ? 2 : 4) * (size_t)channels(); }
    template <class T> T& at(int r, int c) { return reinterpret_cast<T*>(data)[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return reinterpret_cast<const T*>(data)[(size_t)r * cols + c]; }
    template <class T> T& at(int i) { return reinterpret_cast<T*>(data)[i]; }
    template <class T> const T& at(int i) const { return reinterpret_cast<const T*>(data)[i]; }

  private:
    int type_ = 0;
    std::shared_ptr<std::vector<unsigned char> > buf_;
};

void pyrDown(const Mat&, Mat&, const Size&);
void cvtColor(const Mat&, Mat&, int);
void Sobel(const Mat&, Mat&, int, int, int);
void GaussianBlur(const Mat&, Mat&, const Size&, double);
void bilateralFilter(const Mat&, Mat&, int, double, double);
} // namespace cv
